// ecapa.hip -- ECAPA-TDNN speaker embedder of libccx (speechbrain/spkrec-ecapa-voxceleb: C = 1024, 192-d).
// Semantics follow speechbrain's lobes/models/ECAPA_TDNN.py, lobes/features.py::Fbank and InputNormalization [UPSTREAM-RECALL];
// fp64 restatement: tests/ecapa_reference.py.  Eval mode, fixed geometry of the VoxCeleb checkpoint.
//
//   Fbank(80) + sentence mean normalisation -> blocks.0 (TDNN 80 -> 1024, k5) -> 3 x SE-Res2Net(1024, k3, dilation 2 / 3 / 4)
//   -> mfa (TDNN 3072 -> 3072 over the concatenation) -> attentive statistics pooling with global context -> BatchNorm -> fc (192)
//
// Layout (ecapa.h): bf16 [rows][C], every crop with four reflection halo rows on each side, so that `padding="same"` with
// `padding_mode="reflect"` is a plain strided view for blocks.0 and the 1 x 1 TDNNs, the SE scale and the residual add (pointwise in
// time) keep a valid halo valid.  Halos are produced after the front end, after blocks.0 and by the Res2Net kernel.  Reductions over
// time run over the T valid rows of a crop only, and every crop is its own utterance: nothing a crop computes depends on its launch
// mates.  The 1 x 1 TDNNs, blocks.0, mfa, the context projection and fc are GEMMs of the existing family (gemm_bf16.h); the kernels
// here are the front end, the Res2Net chain, squeeze-excitation and the pooling.
#include <math.h>
#include <algorithm>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "ecapa.h"
#include "gemm_bf16.h"
#include "model_store.h"
#include "op_scratch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Front end.  Pass 1 (ecapa_fbank_kernel): a block owns 32 frames of one crop; samples staged in LDS (center=True with ZERO padding),
// one DFT bin per lane against the window-folded tables, power spectrum through LDS into the dense [80][201] mel projection,
// 10 log10(max(x, 1e-10)) to `raw`, the crop's maximum merged with one atomicMax (max is exact: no order dependence).
// Pass 2 (ecapa_fbank_mean_kernel): per (crop, piece) sums of max(raw, crop max - 80) per bin.
// Pass 3 (ecapa_fbank_apply_kernel): combines the pieces in fixed order, subtracts the mean, writes bf16 rows and the halos.
// ---------------------------------------------------------------------------------------------
#define FB_FRAMES 32
#define FB_SPAN (ECAPA_HOP * (FB_FRAMES - 1) + ECAPA_NFFT)
#define FB_PSTRIDE 204
#define FB_DB_OFFSET 128.0f     // raw >= -100 dB, so raw + 128 is a positive float whose bit order is its value order

__global__ __launch_bounds__(256) void ecapa_fbank_kernel(const float* __restrict__ wav, const long* __restrict__ crop_off,
                                                          const int* __restrict__ crop_len, const int* __restrict__ row_off,
                                                          const int* __restrict__ frames, const float* __restrict__ dft_cos,
                                                          const float* __restrict__ dft_sin, const float* __restrict__ filt,
                                                          float* __restrict__ raw, unsigned int* __restrict__ gmax) {
  __shared__ __attribute__((aligned(16))) float xs[FB_SPAN];
  __shared__ __attribute__((aligned(16))) float pw[FB_FRAMES * FB_PSTRIDE];
  __shared__ float red[4];
  const int crop = blockIdx.y, f0 = blockIdx.x * FB_FRAMES, tid = threadIdx.x;
  const int T = frames[crop];
  if (f0 >= T) return;                                             // block-uniform
  const int n = crop_len[crop];
  const float* x = wav + crop_off[crop];
  const long i0 = (long)f0 * ECAPA_HOP - ECAPA_NFFT / 2;
  for (int i = tid; i < FB_SPAN; i += 256) {
    const long o = i0 + i;
    xs[i] = (o >= 0 && o < n) ? x[o] : 0.f;
  }
  __syncthreads();
  float re[FB_FRAMES], im[FB_FRAMES];
#pragma unroll
  for (int f = 0; f < FB_FRAMES; f++) { re[f] = 0.f; im[f] = 0.f; }
  if (tid < ECAPA_BINS) {
    for (int nn = 0; nn < ECAPA_NFFT; nn += 4) {
      float c[4], s[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        c[j] = dft_cos[(nn + j) * ECAPA_BINS_LD + tid];
        s[j] = dft_sin[(nn + j) * ECAPA_BINS_LD + tid];
      }
#pragma unroll
      for (int f = 0; f < FB_FRAMES; f++) {
        const float4 xv = *(const float4*)(xs + f * ECAPA_HOP + nn);
        re[f] = fmaf(xv.x, c[0], re[f]); im[f] = fmaf(xv.x, s[0], im[f]);
        re[f] = fmaf(xv.y, c[1], re[f]); im[f] = fmaf(xv.y, s[1], im[f]);
        re[f] = fmaf(xv.z, c[2], re[f]); im[f] = fmaf(xv.z, s[2], im[f]);
        re[f] = fmaf(xv.w, c[3], re[f]); im[f] = fmaf(xv.w, s[3], im[f]);
      }
    }
#pragma unroll
    for (int f = 0; f < FB_FRAMES; f++) pw[f * FB_PSTRIDE + tid] = re[f] * re[f] + im[f] * im[f];
  }
  __syncthreads();
  // mel projection: 80 x 32 outputs, ten per thread; thread -> frame tid & 31, mel (tid >> 5) + 8 i
  float lmax = -100.f;
  const int f = tid & 31;
  const long orow = (long)row_off[crop] + ECAPA_HALO + f0 + f;
#pragma unroll 1
  for (int i = 0; i < ECAPA_MELS / 8; i++) {
    const int m = (tid >> 5) + 8 * i;
    float acc = 0.f;
    for (int k = 0; k < ECAPA_BINS; k++) acc = fmaf(filt[m * ECAPA_BINS_LD + k], pw[f * FB_PSTRIDE + k], acc);
    const float v = 10.f * log10f(fmaxf(acc, 1e-10f));
    if (f0 + f < T) { raw[orow * ECAPA_MELS + m] = v; lmax = fmaxf(lmax, v); }
  }
  lmax = wave_reduce_max(lmax);
  if ((tid & 63) == 0) red[tid >> 6] = lmax;
  __syncthreads();
  if (tid == 0) {
    const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(gmax + crop, __float_as_uint(mx + FB_DB_OFFSET));
  }
}

__global__ __launch_bounds__(256) void ecapa_fbank_mean_kernel(const float* __restrict__ raw, const unsigned int* __restrict__ gmax,
                                                               const int* __restrict__ row_off, const int* __restrict__ frames,
                                                               float* __restrict__ part) {
  __shared__ float red[3][ECAPA_MELS];
  const int crop = blockIdx.x, piece = blockIdx.y, tid = threadIdx.x;
  const int T = frames[crop], per = (T + ECAPA_PIECES - 1) / ECAPA_PIECES;
  const int t0 = piece * per, t1 = min(T, t0 + per);
  const float floorv = __uint_as_float(gmax[crop]) - FB_DB_OFFSET - 80.f;
  const float* x = raw + ((long)row_off[crop] + ECAPA_HALO) * ECAPA_MELS;
  const int g = tid / ECAPA_MELS, m = tid - g * ECAPA_MELS;
  if (g < 3) {
    float s = 0.f;
    for (int t = t0 + g; t < t1; t += 3) s += fmaxf(x[(long)t * ECAPA_MELS + m], floorv);
    red[g][m] = s;
  }
  __syncthreads();
  if (tid < ECAPA_MELS) part[((long)crop * ECAPA_PIECES + piece) * ECAPA_MELS + tid] = (red[0][tid] + red[1][tid]) + red[2][tid];
}

// rows a frame t of a T-frame crop is written to besides its own: the halo rows that mirror it (t = 1..4 -> -t; T-1-t = 1..4 -> 2(T-1)-t)
__device__ __forceinline__ int ecapa_mirror_lo(int t) { return (t >= 1 && t <= ECAPA_HALO) ? -t : 0; }
__device__ __forceinline__ int ecapa_mirror_hi(int t, int T) { const int j = T - 1 - t; return (j >= 1 && j <= ECAPA_HALO) ? T - 1 + j : 0; }

__global__ __launch_bounds__(256) void ecapa_fbank_apply_kernel(const float* __restrict__ raw, const unsigned int* __restrict__ gmax,
                                                                const int* __restrict__ row_off, const int* __restrict__ frames,
                                                                const float* __restrict__ part, bf16_t* __restrict__ feats) {
  __shared__ float mean[ECAPA_MELS];
  const int crop = blockIdx.x, piece = blockIdx.y, tid = threadIdx.x;
  const int T = frames[crop], per = (T + ECAPA_PIECES - 1) / ECAPA_PIECES;
  const int t0 = piece * per, t1 = min(T, t0 + per);
  if (t0 >= t1) return;                                            // block-uniform
  if (tid < ECAPA_MELS) {
    float s = 0.f;
    for (int i = 0; i < ECAPA_PIECES; i++) s += part[((long)crop * ECAPA_PIECES + i) * ECAPA_MELS + tid];
    mean[tid] = s / (float)T;
  }
  __syncthreads();
  const float floorv = __uint_as_float(gmax[crop]) - FB_DB_OFFSET - 80.f;
  const long r0 = (long)row_off[crop] + ECAPA_HALO;
  for (int i = tid; i < (t1 - t0) * ECAPA_MELS; i += 256) {
    const int t = t0 + i / ECAPA_MELS, m = i % ECAPA_MELS;
    const bf16_t v = f32_to_bf16(fmaxf(raw[(r0 + t) * ECAPA_MELS + m], floorv) - mean[m]);
    feats[(r0 + t) * ECAPA_MELS + m] = v;
    const int lo = ecapa_mirror_lo(t), hi = ecapa_mirror_hi(t, T);
    if (lo) feats[(r0 + lo) * ECAPA_MELS + m] = v;
    if (hi) feats[(r0 + hi) * ECAPA_MELS + m] = v;
  }
}

// reflection halos of a [rows][ld] buffer: grid (crops, 8 halo rows), 16-byte pieces of C columns
__global__ __launch_bounds__(128) void ecapa_halo_kernel(bf16_t* __restrict__ buf, long ld, int C, const int* __restrict__ row_off,
                                                         const int* __restrict__ frames) {
  const int crop = blockIdx.x, h = blockIdx.y, T = frames[crop];
  const int j = (h & 3) + 1;
  const int dst = h < 4 ? -j : T - 1 + j, src = h < 4 ? j : T - 1 - j;
  const long r0 = (long)row_off[crop] + ECAPA_HALO;
  const uint4* s = (const uint4*)(buf + (r0 + src) * ld);
  uint4* d = (uint4*)(buf + (r0 + dst) * ld);
  for (int i = threadIdx.x; i < C / 8; i += 128) d[i] = s[i];
}

// ---------------------------------------------------------------------------------------------
// Res2Net chain of one SE-Res2Net block: y0 = x0, y1 = B0(x1), yi = B(i-1)(xi + y(i-1)), each B = Conv1d(128 -> 128, k3, dilation d,
// reflect) -> ReLU -> BatchNorm.  One block computes all seven stages of a (crop, tile of F = 128 frames):
//   * stage s is needed on the tile widened by (7 - s) d frames on each side (the time halo is recomputed), clipped to the crop;
//   * a stage's input z = x_s + y_(s-1) lives in LDS as bf16 (two buffers, ping-pong; 288-byte rows as in the LSTM kernel: conflict-free
//     ds_read_b128), indexed by position; the reflection is applied to EVERY stage's input by index (q < 0 -> -q, q > T-1 ->
//     2 (T-1) - q), so the kernel never reads a halo row of x;
//   * the MFMA runs over the three taps, K = 3 x 128 per stage.  The weights are the A operand and the activations the B operand, so a
//     lane's four accumulators are four CONSECUTIVE CHANNELS of one frame: x is fetched and y stored in 8-byte pieces, and the next
//     stage's input goes to LDS in 8-byte pieces.  Wave w owns output channels 16 w .. 16 w + 15; its 12 weight fragments of a stage
//     (packed at finalize in fragment order, 96 KB per stage for the block: too much to sit in LDS beside the tiles) come through L2 into
//     registers once per stage;
//   * chunk 0 is copied through, and every stored frame also goes to the halo rows that mirror it.
// ---------------------------------------------------------------------------------------------
#define R2_ROWS (ECAPA_R2_TILE + 2 * ECAPA_R2_MARGIN)
#define R2_LD 144
#define R2_LDS (2 * R2_ROWS * R2_LD * 2)

__device__ __forceinline__ void r2_store_row(bf16_t* __restrict__ y, long ldy, long r0, int p, int T, int col, uint2 v) {
  *(uint2*)(y + (r0 + p) * ldy + col) = v;
  const int lo = ecapa_mirror_lo(p), hi = ecapa_mirror_hi(p, T);
  if (lo) *(uint2*)(y + (r0 + lo) * ldy + col) = v;
  if (hi) *(uint2*)(y + (r0 + hi) * ldy + col) = v;
}

__global__ __launch_bounds__(512) void ecapa_res2net_kernel(const bf16_t* __restrict__ x, long ldx, bf16_t* __restrict__ y, long ldy,
                                                            const int* __restrict__ row_off, const int* __restrict__ frames,
                                                            const bf16_t* __restrict__ wfrag, const float* __restrict__ aff, int d) {
  extern __shared__ __attribute__((aligned(16))) char sm_raw[];
  bf16_t* const Z0 = (bf16_t*)sm_raw;                               // two stage-input buffers of R2_ROWS x R2_LD, ping-pong
  const int crop = blockIdx.y, T = frames[crop], t0 = blockIdx.x * ECAPA_R2_TILE;
  if (t0 >= T) return;                                             // block-uniform
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, hq = lane >> 4;
  const int t1 = min(T, t0 + ECAPA_R2_TILE);                        // the tile's frames are [t0, t1)
  const long r0 = (long)row_off[crop] + ECAPA_HALO;                 // row of frame 0
  const int pb = t0 - ECAPA_R2_MARGIN;                              // position of LDS row 0
  // chunk 0: copied through
  for (int i = tid; i < (t1 - t0) * 32; i += 512) {
    const int p = t0 + (i >> 5), c = (i & 31) * 4;
    r2_store_row(y, ldy, r0, p, T, c, *(const uint2*)(x + (r0 + p) * ldx + c));
  }
  // stage 1 input: chunk 1 on the tile widened by 7 d
  {
    const int lo = max(0, t0 - ECAPA_R2_STAGES * d), hi = min(T - 1, t0 + ECAPA_R2_TILE - 1 + ECAPA_R2_STAGES * d);
    for (int i = tid; i < (hi - lo + 1) * 16; i += 512) {
      const int p = lo + (i >> 4), c = (i & 15) * 8;
      *(uint4*)(Z0 + (p - pb) * R2_LD + c) = *(const uint4*)(x + (r0 + p) * ldx + 128 + c);
    }
  }
  __syncthreads();
  const int ch = 16 * wave + 4 * hq;                                // this lane's four output channels
#pragma unroll 1
  for (int s = 1; s <= ECAPA_R2_STAGES; s++) {
    const bf16_t* cur = Z0 + ((s - 1) & 1) * (R2_ROWS * R2_LD);
    bf16_t* nxt = Z0 + (s & 1) * (R2_ROWS * R2_LD);
    const int lo = max(0, t0 - (ECAPA_R2_STAGES - s) * d), hi = min(T - 1, t0 + ECAPA_R2_TILE - 1 + (ECAPA_R2_STAGES - s) * d);
    bf16x8 wf[3][4];
#pragma unroll
    for (int tap = 0; tap < 3; tap++)
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
        wf[tap][ks] = *(const bf16x8*)(wfrag + ((((long)(s - 1) * 3 + tap) * 4 + ks) * 8 + wave) * 512 + lane * 8);
    const float4 bia = *(const float4*)(aff + ((s - 1) * 3 + 0) * 128 + ch), sc = *(const float4*)(aff + ((s - 1) * 3 + 1) * 128 + ch),
                 sh = *(const float4*)(aff + ((s - 1) * 3 + 2) * 128 + ch);
    const int ntile = (hi - lo + 16) >> 4;
#pragma unroll 1
    for (int mt = 0; mt < ntile; mt++) {
      const int p = lo + 16 * mt + l15, pr = min(p, hi);            // rows past `hi` recompute row `hi` and store nothing
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tap = 0; tap < 3; tap++) {
        int q = pr + (tap - 1) * d;
        q = q < 0 ? -q : q;
        q = q > T - 1 ? 2 * (T - 1) - q : q;
        const bf16_t* zr = cur + (q - pb) * R2_LD + 8 * hq;
#pragma unroll
        for (int ks = 0; ks < 4; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tap][ks], *(const bf16x8*)(zr + 32 * ks), acc, 0, 0, 0);
      }
      if (p <= hi) {
        const float v0 = fmaxf(acc[0] + bia.x, 0.f) * sc.x + sh.x, v1 = fmaxf(acc[1] + bia.y, 0.f) * sc.y + sh.y,
                    v2 = fmaxf(acc[2] + bia.z, 0.f) * sc.z + sh.z, v3 = fmaxf(acc[3] + bia.w, 0.f) * sc.w + sh.w;
        if (p >= t0 && p < t1) {
          uint2 pk;
          pk.x = pack_bf16x2(v0, v1); pk.y = pack_bf16x2(v2, v3);
          r2_store_row(y, ldy, r0, p, T, s * 128 + ch, pk);
        }
        if (s < ECAPA_R2_STAGES) {
          const uint2 xv = *(const uint2*)(x + (r0 + p) * ldx + (s + 1) * 128 + ch);
          uint2 pk;
          pk.x = pack_bf16x2(v0 + bf16_to_f32((bf16_t)(xv.x & 0xffff)), v1 + bf16_to_f32((bf16_t)(xv.x >> 16)));
          pk.y = pack_bf16x2(v2 + bf16_to_f32((bf16_t)(xv.y & 0xffff)), v3 + bf16_to_f32((bf16_t)(xv.y >> 16)));
          *(uint2*)(nxt + (p - pb) * R2_LD + ch) = pk;
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Column statistics of a crop over its valid rows: mean (SE) or mean and std = sqrt(max(sum (x - mean)^2 / T, 1e-12)) (context of the
// pooling).  grid (crops, C / 256); 256 threads = 64 channel quads x 4 interleaved row groups, combined in fixed order.
// ---------------------------------------------------------------------------------------------
template <bool STD>
__global__ __launch_bounds__(256) void ecapa_col_stats_kernel(const bf16_t* __restrict__ x, long ld, const int* __restrict__ row_off,
                                                              const int* __restrict__ frames, float* __restrict__ out, int C) {
  __shared__ float4 red[4][64];
  const int crop = blockIdx.x, q = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.y * 256 + 4 * q;
  const int T = frames[crop];
  const bf16_t* p = x + ((long)row_off[crop] + ECAPA_HALO) * ld + c;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = g; t < T; t += 4) {
    const uint2 v = *(const uint2*)(p + (long)t * ld);
    s.x += bf16_to_f32((bf16_t)(v.x & 0xffff)); s.y += bf16_to_f32((bf16_t)(v.x >> 16));
    s.z += bf16_to_f32((bf16_t)(v.y & 0xffff)); s.w += bf16_to_f32((bf16_t)(v.y >> 16));
  }
  red[g][q] = s;
  __syncthreads();
  const float inv = 1.f / (float)T;
  float4 mean;
  mean.x = ((red[0][q].x + red[1][q].x) + (red[2][q].x + red[3][q].x)) * inv;
  mean.y = ((red[0][q].y + red[1][q].y) + (red[2][q].y + red[3][q].y)) * inv;
  mean.z = ((red[0][q].z + red[1][q].z) + (red[2][q].z + red[3][q].z)) * inv;
  mean.w = ((red[0][q].w + red[1][q].w) + (red[2][q].w + red[3][q].w)) * inv;
  float* o = out + (long)crop * (STD ? 2 * C : C);
  if (g == 0) *(float4*)(o + c) = mean;
  if (!STD) return;
  __syncthreads();
  float4 m2 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = g; t < T; t += 4) {
    const uint2 v = *(const uint2*)(p + (long)t * ld);
    const float a = bf16_to_f32((bf16_t)(v.x & 0xffff)) - mean.x, b = bf16_to_f32((bf16_t)(v.x >> 16)) - mean.y,
                e = bf16_to_f32((bf16_t)(v.y & 0xffff)) - mean.z, f = bf16_to_f32((bf16_t)(v.y >> 16)) - mean.w;
    m2.x += a * a; m2.y += b * b; m2.z += e * e; m2.w += f * f;
  }
  red[g][q] = m2;
  __syncthreads();
  if (g == 0) {
    float4 sd;
    sd.x = sqrtf(fmaxf(((red[0][q].x + red[1][q].x) + (red[2][q].x + red[3][q].x)) * inv, 1e-12f));
    sd.y = sqrtf(fmaxf(((red[0][q].y + red[1][q].y) + (red[2][q].y + red[3][q].y)) * inv, 1e-12f));
    sd.z = sqrtf(fmaxf(((red[0][q].z + red[1][q].z) + (red[2][q].z + red[3][q].z)) * inv, 1e-12f));
    sd.w = sqrtf(fmaxf(((red[0][q].w + red[1][q].w) + (red[2][q].w + red[3][q].w)) * inv, 1e-12f));
    *(float4*)(o + C + c) = sd;
  }
}

// SE gates of one crop, fp32: e = sigmoid(W2 relu(W1 mean + b1) + b2), W1 [128][1024], W2 [1024][128]
__global__ __launch_bounds__(256) void ecapa_se_excite_kernel(const float* __restrict__ mean, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float* __restrict__ gates) {
  __shared__ __attribute__((aligned(16))) float ms[1024];
  __shared__ __attribute__((aligned(16))) float hs[128];
  const int crop = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 1024; i += 256) ms[i] = mean[(long)crop * 1024 + i];
  __syncthreads();
  for (int j = wave; j < 128; j += 4) {
    const float* w = w1 + (long)j * 1024;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float4 a = *(const float4*)(w + 256 * k + 4 * lane), b = *(const float4*)(ms + 256 * k + 4 * lane);
      s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
    }
    s = wave_reduce_sum(s);
    if (lane == 0) hs[j] = fmaxf(s + b1[j], 0.f);
  }
  __syncthreads();
  for (int c = tid; c < 1024; c += 256) {
    const float* w = w2 + (long)c * 128;
    float s = b2[c];
#pragma unroll 8
    for (int k = 0; k < 128; k += 4) {
      const float4 a = *(const float4*)(w + k), b = *(const float4*)(hs + k);
      s = fmaf(a.x, b.x, s); s = fmaf(a.y, b.y, s); s = fmaf(a.z, b.z, s); s = fmaf(a.w, b.w, s);
    }
    gates[(long)crop * 1024 + c] = 1.f / (1.f + expf(-s));
  }
}

// y = gates * x + resid over ALL rows of a crop (the halos stay valid: pointwise in time).  grid (crops, 16 pieces)
__global__ __launch_bounds__(256) void ecapa_se_apply_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ resid,
                                                             long ldr, bf16_t* __restrict__ y, long ldy, const int* __restrict__ row_off,
                                                             const int* __restrict__ frames, const float* __restrict__ gates) {
  const int crop = blockIdx.x, piece = blockIdx.y;
  const int R = frames[crop] + 2 * ECAPA_HALO, per = (R + ECAPA_PIECES - 1) / ECAPA_PIECES;
  const int a = piece * per, b = min(R, a + per);
  const long r0 = row_off[crop];
  const float* e = gates + (long)crop * 1024;
  for (int i = threadIdx.x; i < (b - a) * 128; i += 256) {
    const int r = a + (i >> 7), c = (i & 127) * 8;
    const uint4 xv = *(const uint4*)(x + (r0 + r) * ldx + c), rv = *(const uint4*)(resid + (r0 + r) * ldr + c);
    const float4 e0 = *(const float4*)(e + c), e1 = *(const float4*)(e + c + 4);
    const uint32_t xs[4] = {xv.x, xv.y, xv.z, xv.w}, rs[4] = {rv.x, rv.y, rv.z, rv.w};
    const float es[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float lo = fmaf(es[2 * k], bf16_to_f32((bf16_t)(xs[k] & 0xffff)), bf16_to_f32((bf16_t)(rs[k] & 0xffff)));
      const float hi = fmaf(es[2 * k + 1], bf16_to_f32((bf16_t)(xs[k] >> 16)), bf16_to_f32((bf16_t)(rs[k] >> 16)));
      o[k] = pack_bf16x2(lo, hi);
    }
    *(uint4*)(y + (r0 + r) * ldy + c) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// context term of the attention's TDNN, by linearity W [x; mean; std] = W_x x + (W_m mean + W_s std + b): the bracket, per crop.
// stat f32 [n][6144] (mean | std), wms f32 [128][6144], out f32 [n][128]
__global__ __launch_bounds__(256) void ecapa_ctx_vec_kernel(const float* __restrict__ stat, const float* __restrict__ wms,
                                                            const float* __restrict__ b, float* __restrict__ out) {
  const int crop = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* sv = stat + (long)crop * 6144;
  for (int j = wave; j < 128; j += 4) {
    const float* w = wms + (long)j * 6144;
    float s = 0.f;
    for (int k = 4 * lane; k < 6144; k += 256) {
      const float4 a = *(const float4*)(w + k), v = *(const float4*)(sv + k);
      s = fmaf(a.x, v.x, s); s = fmaf(a.y, v.y, s); s = fmaf(a.z, v.z, s); s = fmaf(a.w, v.w, s);
    }
    s = wave_reduce_sum(s);
    if (lane == 0) out[(long)crop * 128 + j] = s + b[j];
  }
}

// hidden = tanh(BatchNorm(relu(W_x x + crop vector))) -> bf16 [rows][128], valid rows only.  grid (crops, 16 pieces)
__global__ __launch_bounds__(256) void ecapa_asp_hidden_kernel(const float* __restrict__ h32, const float* __restrict__ cvec,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const int* __restrict__ row_off, const int* __restrict__ frames,
                                                               bf16_t* __restrict__ hidden) {
  const int crop = blockIdx.x, piece = blockIdx.y;
  const int T = frames[crop], per = (T + ECAPA_PIECES - 1) / ECAPA_PIECES;
  const int a = piece * per, b = min(T, a + per);
  const long r0 = (long)row_off[crop] + ECAPA_HALO;
  for (int i = threadIdx.x; i < (b - a) * 128; i += 256) {
    const int t = a + (i >> 7), c = i & 127;
    const float v = fmaxf(h32[(r0 + t) * 128 + c] + cvec[(long)crop * 128 + c], 0.f) * scale[c] + shift[c];
    hidden[(r0 + t) * 128 + c] = f32_to_bf16(tanhf(v));
  }
}

// ---------------------------------------------------------------------------------------------
// Attentive statistics pooling.  grid (crops, C / 64); a wave owns 16 channels and walks the crop's frames 16 at a time: the logits
// of a (16 frames x 16 channels) tile are ONE accumulator (hidden rows as the A operand, the 16 x 128 slice of the attention weights
// as four B fragments held in registers, K = 128), so a lane sees four frames of ONE channel and the [rows][C] logits never exist in
// memory.  Two passes that recompute the logits:
//   pass 1: online softmax over the lane's frames (max m, Z = sum e^(l - m), S = sum e^(l - m) x), merged over the four lane groups
//           of a channel -> the weighted mean;
//   pass 2: sum e^(l - M) (x - mean)^2 with the final M -> the variance in the reference's own form.  (One online pass would need
//           E[x^2] - mean^2, which cancels for a channel of large mean and tiny variance.)
// Epilogue: std = sqrt(max(var, 1e-12)), asp_bn's affine, bf16 -> out [n][2 C] (mean | std).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float asp_group_max(float v) { v = fmaxf(v, lane_xor16(v)); return fmaxf(v, lane_xor32(v)); }
__device__ __forceinline__ float asp_group_sum(float v) { v += lane_xor16(v); return v + lane_xor32(v); }

__global__ __launch_bounds__(256) void ecapa_asp_pool_kernel(const bf16_t* __restrict__ hidden, const bf16_t* __restrict__ x, long ldx,
                                                             const int* __restrict__ row_off, const int* __restrict__ frames,
                                                             const bf16_t* __restrict__ wa, const float* __restrict__ ba,
                                                             const float* __restrict__ bn_scale, const float* __restrict__ bn_shift,
                                                             bf16_t* __restrict__ out, int C) {
  const int crop = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, hq = lane >> 4;
  const int c = blockIdx.y * 64 + 16 * wave + l15;
  const int T = frames[crop];
  const long r0 = (long)row_off[crop] + ECAPA_HALO;
  bf16x8 wf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ks++) wf[ks] = *(const bf16x8*)(wa + (long)c * 128 + 32 * ks + 8 * hq);
  const float bias = ba[c];
  const bf16_t* xc = x + r0 * ldx + c;
  constexpr float NEG = -1e30f;
  float m = NEG, Z = 0.f, S = 0.f;
  for (int tt = 0; tt < T; tt += 16) {
    const bf16_t* hr = hidden + (r0 + min(tt + l15, T - 1)) * 128 + 8 * hq;   // frames past the crop re-read its last row, masked below
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(hr + 32 * ks), wf[ks], acc, 0, 0, 0);
    float l[4], xv[4], tm = NEG;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int t = tt + 4 * hq + r;
      const bool ok = t < T;
      l[r] = ok ? acc[r] + bias : NEG;
      xv[r] = ok ? bf16_to_f32(xc[(long)t * ldx]) : 0.f;
      tm = fmaxf(tm, l[r]);
    }
    if (tm > m) { const float f = expf(m - tm); Z *= f; S *= f; m = tm; }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float e = l[r] > 0.5f * NEG ? expf(l[r] - m) : 0.f;
      Z += e; S = fmaf(e, xv[r], S);
    }
  }
  const float M = asp_group_max(m);
  const float f = m > 0.5f * NEG ? expf(m - M) : 0.f;
  const float Zt = asp_group_sum(Z * f);
  const float mean = asp_group_sum(S * f) / Zt;
  float V = 0.f;
  for (int tt = 0; tt < T; tt += 16) {
    const bf16_t* hr = hidden + (r0 + min(tt + l15, T - 1)) * 128 + 8 * hq;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(hr + 32 * ks), wf[ks], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int t = tt + 4 * hq + r;
      if (t < T) {
        const float dv = bf16_to_f32(xc[(long)t * ldx]) - mean;
        V = fmaf(expf(acc[r] + bias - M), dv * dv, V);
      }
    }
  }
  const float var = asp_group_sum(V) / Zt;
  if (hq == 0) {
    const float sd = sqrtf(fmaxf(var, 1e-12f));
    out[(long)crop * 2 * C + c] = f32_to_bf16(mean * bn_scale[c] + bn_shift[c]);
    out[(long)crop * 2 * C + C + c] = f32_to_bf16(sd * bn_scale[C + c] + bn_shift[C + c]);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
void ccx_ecapa_fbank_tables(const float* window, const float* filters, std::vector<float>& dft_cos, std::vector<float>& dft_sin,
                            std::vector<float>& filt) {
  dft_cos.assign((size_t)ECAPA_NFFT * ECAPA_BINS_LD, 0.f);
  dft_sin.assign((size_t)ECAPA_NFFT * ECAPA_BINS_LD, 0.f);
  filt.assign((size_t)ECAPA_MELS * ECAPA_BINS_LD, 0.f);
  for (int n = 0; n < ECAPA_NFFT; n++)
    for (int k = 0; k < ECAPA_BINS; k++) {
      const double a = 2.0 * M_PI * (double)((n * k) % ECAPA_NFFT) / ECAPA_NFFT;
      dft_cos[(size_t)n * ECAPA_BINS_LD + k] = (float)((double)window[n] * cos(a));
      dft_sin[(size_t)n * ECAPA_BINS_LD + k] = (float)((double)window[n] * sin(a));
    }
  for (int m = 0; m < ECAPA_MELS; m++)
    for (int k = 0; k < ECAPA_BINS; k++) filt[(size_t)m * ECAPA_BINS_LD + k] = filters[(size_t)m * ECAPA_BINS + k];
}

void ccx_ecapa_pack_res2net(const float* w, std::vector<float>& frag) {
  frag.assign((size_t)ECAPA_R2_STAGES * ECAPA_R2_WFRAG, 0.f);
  for (int s = 0; s < ECAPA_R2_STAGES; s++)
    for (int tap = 0; tap < 3; tap++)
      for (int ks = 0; ks < 4; ks++)
        for (int nt = 0; nt < 8; nt++)
          for (int lane = 0; lane < 64; lane++)
            for (int e = 0; e < 8; e++) {
              const int o = 16 * nt + (lane & 15), k = 32 * ks + 8 * (lane >> 4) + e;
              frag[(((((size_t)s * 3 + tap) * 4 + ks) * 8 + nt) * 64 + lane) * 8 + e] = w[(((size_t)s * 128 + o) * 128 + k) * 3 + tap];
            }
}

int ccx_launch_ecapa_fbank(ccx_ctx* ctx, const float* wav, const long* crop_off, const int* crop_len, const EcapaCrops& cr,
                           const float* dft_cos, const float* dft_sin, const float* filt, float* raw, unsigned int* gmax, float* part,
                           bf16_t* feats, hipStream_t st) {
  CCX_HIP(ctx, hipMemsetAsync(gmax, 0, (size_t)cr.n * sizeof(unsigned int), st));   // 0.0f: below every raw + 128
  {
    const double fr = (double)cr.n * cr.max_frames;
    ccx_prof_scope ps(ctx, st, "ecapa_fbank_kernel", fr * (4.0 * ECAPA_NFFT * ECAPA_BINS + 2.0 * ECAPA_MELS * ECAPA_BINS),
                      fr * (4.0 * ECAPA_HOP + 4.0 * ECAPA_MELS));
    hipLaunchKernelGGL(ecapa_fbank_kernel, dim3(ccx_cdiv(cr.max_frames, FB_FRAMES), cr.n), dim3(256), 0, st, wav, crop_off, crop_len,
                       cr.row_off, cr.frames, dft_cos, dft_sin, filt, raw, gmax);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "ecapa_fbank_mean_kernel", 2.0 * cr.n * cr.max_frames * ECAPA_MELS, 4.0 * cr.n * cr.max_frames * ECAPA_MELS);
    hipLaunchKernelGGL(ecapa_fbank_mean_kernel, dim3(cr.n, ECAPA_PIECES), dim3(256), 0, st, raw, gmax, cr.row_off, cr.frames, part);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "ecapa_fbank_apply_kernel", 2.0 * cr.n * cr.max_frames * ECAPA_MELS, 6.0 * cr.n * cr.max_frames * ECAPA_MELS);
    hipLaunchKernelGGL(ecapa_fbank_apply_kernel, dim3(cr.n, ECAPA_PIECES), dim3(256), 0, st, raw, gmax, cr.row_off, cr.frames, part, feats);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_ecapa_halo(ccx_ctx* ctx, bf16_t* buf, long ld, int C, const EcapaCrops& cr, hipStream_t st) {
  ccx_prof_scope ps(ctx, st, "ecapa_halo_kernel", 0.0, 32.0 * cr.n * C);
  hipLaunchKernelGGL(ecapa_halo_kernel, dim3(cr.n, 2 * ECAPA_HALO), dim3(128), 0, st, buf, ld, C, cr.row_off, cr.frames);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_ecapa_res2net(ccx_ctx* ctx, const bf16_t* x, long ldx, bf16_t* y, long ldy, const EcapaCrops& cr, const bf16_t* wfrag,
                             const float* aff, int dilation, hipStream_t st) {
  CCX_REQUIRE(ctx, dilation >= 1 && dilation * ECAPA_R2_STAGES <= ECAPA_R2_MARGIN, "ecapa res2net: dilation = %d out of range [1, 4]", dilation);
  static ccx_lds_optin optin;
  CCX_HIP(ctx, optin.ensure(ctx->device, (const void*)ecapa_res2net_kernel, R2_LDS));
  const int tiles = ccx_cdiv(cr.max_frames, ECAPA_R2_TILE);
  const double fr = (double)cr.n * cr.max_frames;
  ccx_prof_scope ps(ctx, st, "ecapa_res2net_kernel", fr * ECAPA_R2_STAGES * 2.0 * 128 * 384, fr * 1024 * 4.0 + (double)cr.n * tiles * ECAPA_R2_STAGES * ECAPA_R2_WFRAG * 2.0);
  hipLaunchKernelGGL(ecapa_res2net_kernel, dim3(tiles, cr.n), dim3(512), R2_LDS, st, x, ldx, y, ldy, cr.row_off, cr.frames, wfrag, aff, dilation);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_ecapa_se(ccx_ctx* ctx, const bf16_t* x, long ldx, const bf16_t* resid, long ldr, bf16_t* y, long ldy, const EcapaCrops& cr,
                        const float* w1, const float* b1, const float* w2, const float* b2, float* mean, float* gates, hipStream_t st) {
  const double el = (double)cr.n * cr.max_frames * 1024;
  {
    ccx_prof_scope ps(ctx, st, "ecapa_se_mean_kernel", el, 2.0 * el);
    hipLaunchKernelGGL(ecapa_col_stats_kernel<false>, dim3(cr.n, 4), dim3(256), 0, st, x, ldx, cr.row_off, cr.frames, mean, 1024);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "ecapa_se_excite_kernel", 4.0 * cr.n * 128 * 1024, 8.0 * 128 * 1024);
    hipLaunchKernelGGL(ecapa_se_excite_kernel, dim3(cr.n), dim3(256), 0, st, mean, w1, b1, w2, b2, gates);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, st, "ecapa_se_apply_kernel", 2.0 * el, 6.0 * el);
    hipLaunchKernelGGL(ecapa_se_apply_kernel, dim3(cr.n, ECAPA_PIECES), dim3(256), 0, st, x, ldx, resid, ldr, y, ldy, cr.row_off, cr.frames, gates);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_ecapa_ctx_stats(ccx_ctx* ctx, const bf16_t* x, long ldx, int C, const EcapaCrops& cr, float* stat, hipStream_t st) {
  CCX_REQUIRE(ctx, C >= 256 && C % 256 == 0, "ecapa ctx stats: C = %d must be a multiple of 256", C);
  const double el = (double)cr.n * cr.max_frames * C;
  ccx_prof_scope ps(ctx, st, "ecapa_ctx_stats_kernel", 4.0 * el, 4.0 * el);
  hipLaunchKernelGGL(ecapa_col_stats_kernel<true>, dim3(cr.n, C / 256), dim3(256), 0, st, x, ldx, cr.row_off, cr.frames, stat, C);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_ecapa_asp_pool(ccx_ctx* ctx, const bf16_t* hidden, const bf16_t* x, long ldx, int C, const EcapaCrops& cr, const bf16_t* wa,
                              const float* ba, const float* bn_scale, const float* bn_shift, bf16_t* out, hipStream_t st) {
  CCX_REQUIRE(ctx, C >= 64 && C % 64 == 0, "ecapa asp pool: channels = %d must be a multiple of 64", C);
  const double el = (double)cr.n * cr.max_frames * C;
  ccx_prof_scope ps(ctx, st, "ecapa_asp_pool_kernel", el * (2.0 * 2.0 * 128 + 10.0), 4.0 * el + 2.0 * (double)cr.n * cr.max_frames * 128 * (C / 64));
  hipLaunchKernelGGL(ecapa_asp_pool_kernel, dim3(cr.n, C / 64), dim3(256), 0, st, hidden, x, ldx, cr.row_off, cr.frames, wa, ba, bn_scale, bn_shift, out, C);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// ---------------------------------------------------------------------------------------------
// the handle
// ---------------------------------------------------------------------------------------------
namespace {
struct EcapaPlan {
  std::vector<long> coff;
  std::vector<int> clen, roff, fr;
};
struct Tdnn { bf16_t* W = nullptr; float *b = nullptr, *sc = nullptr, *sh = nullptr; };
}  // namespace

struct ccx_ecapa {
  ccx_ctx* ctx = nullptr;
  int max_crops = 0;
  long max_samples = 0, Rcap = 0;
  bool finalized = false;
  ccx_dev_store store{"ecapa"};
  float *dft_cos = nullptr, *dft_sin = nullptr, *filt = nullptr;
  Tdnn b0, t1[3], t2[3], mfa;
  bf16_t* r2w[3] = {}; float* r2aff[3] = {};
  float *sw1[3] = {}, *sb1[3] = {}, *sw2[3] = {}, *sb2[3] = {};
  bf16_t* Wx = nullptr; float *wms = nullptr, *basp = nullptr, *asc = nullptr, *ash = nullptr;
  bf16_t* wa = nullptr; float *ba = nullptr, *bnsc = nullptr, *bnsh = nullptr;
  bf16_t* Wfc = nullptr; float* bfc = nullptr;
  // workspaces
  float *raw = nullptr, *fpart = nullptr, *semean = nullptr, *gates = nullptr, *stat = nullptr, *cvec = nullptr, *h32 = nullptr;
  unsigned int* gmax = nullptr;
  bf16_t *feats = nullptr, *a0 = nullptr, *u = nullptr, *v = nullptr, *w = nullptr, *cat = nullptr, *m = nullptr, *hid = nullptr, *pooled = nullptr;
  long* crop_off = nullptr; int *crop_len = nullptr, *row_off = nullptr, *frames = nullptr;
  EcapaPlan plan_ring[4];   // the uploads are asynchronous: the last calls' host tables stay alive here
  int plan_slot = 0;
};

namespace {

// BatchNorm (running statistics, eps 1e-5) folded to scale and shift
int fold_bn(ccx_ecapa* e, const std::string& p, int C, std::vector<float>& sc, std::vector<float>& sh) {
  CCX_NEED(e->store, g, p + ".weight", C); CCX_NEED(e->store, be, p + ".bias", C);
  CCX_NEED(e->store, rm, p + ".running_mean", C); CCX_NEED(e->store, rv, p + ".running_var", C);
  sc.resize(C); sh.resize(C);
  for (int c = 0; c < C; c++) { sc[c] = g->data[c] / sqrtf(rv->data[c] + 1e-5f); sh[c] = be->data[c] - rm->data[c] * sc[c]; }
  return CCX_OK;
}

// TDNNBlock with a 1 x 1 convolution: GEMM weight [O][I] + bias + folded BatchNorm
int load_tdnn(ccx_ecapa* e, const std::string& p, int O, int I, Tdnn& t) {
  CCX_NEED(e->store, w, p + ".conv.conv.weight", (int64_t)O * I); CCX_NEED(e->store, b, p + ".conv.conv.bias", O);
  std::vector<float> sc, sh;
  CCX_TRY(fold_bn(e, p + ".norm.norm", O, sc, sh));
  CCX_TRY(e->store.upload_bf16(&t.W, w->data)); CCX_TRY(e->store.upload(&t.b, b->data.data(), O));
  CCX_TRY(e->store.upload(&t.sc, sc)); CCX_TRY(e->store.upload(&t.sh, sh));
  return CCX_OK;
}

int gemm_tdnn(ccx_ctx* ctx, const Tdnn& t, const bf16_t* A, long lda, int M, int N, int K, bf16_t* out, long ldo, hipStream_t st) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.lda = lda; p.W = t.W; p.ldw = K; p.M = M; p.N = N; p.K = K; p.bias = t.b; p.out = out; p.ldo = ldo;
  p.scale = t.sc; p.shift = t.sh; p.slope = 0.f;      // slope 0: ReLU, then the BatchNorm affine
  return ccx_launch_gemm(ctx, EPI_BF16_LRELU_AFFINE, p, st);
}

}  // namespace

extern "C" {

int ccx_ecapa_create(ccx_ctx* ctx, int max_crops, int64_t max_samples, ccx_ecapa** out) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, out && max_crops >= 1 && max_samples >= ECAPA_MIN_SAMPLES, "ccx_ecapa_create: capacity too small");
  ccx_ecapa* e = new ccx_ecapa();
  e->ctx = ctx; e->store.ctx = ctx; e->max_crops = max_crops; e->max_samples = max_samples;
  *out = e;
  return CCX_OK;
}

void ccx_ecapa_destroy(ccx_ecapa* e) {
  if (!e) return;
  e->store.free_all();
  delete e;
}

int ccx_ecapa_set_tensor(ccx_ecapa* e, const char* name, const float* data, int64_t numel) {
  if (!e) return CCX_ERR_ARG;
  CCX_REQUIRE(e->ctx, !e->finalized && name && data && numel > 0, "ecapa: set_tensor bad arguments");
  return e->store.stage(name, data, numel);
}

int ccx_ecapa_finalize(ccx_ecapa* e) {
  if (!e) return CCX_ERR_ARG;
  CCX_REQUIRE(e->ctx, !e->finalized, "ecapa: finalize called twice");
  ccx_dev_store& S = e->store;
  {
    CCX_NEED(S, win, "fbank.window", ECAPA_NFFT); CCX_NEED(S, fb, "fbank.filters", ECAPA_MELS * ECAPA_BINS);
    std::vector<float> dc, ds, fl;
    ccx_ecapa_fbank_tables(win->data.data(), fb->data.data(), dc, ds, fl);
    CCX_TRY(S.upload(&e->dft_cos, dc)); CCX_TRY(S.upload(&e->dft_sin, ds)); CCX_TRY(S.upload(&e->filt, fl));
  }
  {  // blocks.0: Conv1d(80 -> 1024, k5) as one GEMM over the 5-frame view, K = 400 -> 448
    CCX_NEED(S, w, "blocks.0.conv.conv.weight", 1024 * 80 * 5); CCX_NEED(S, b, "blocks.0.conv.conv.bias", 1024);
    std::vector<float> wp((size_t)1024 * 448, 0.f), sc, sh;
    for (int o = 0; o < 1024; o++)
      for (int c = 0; c < 80; c++)
        for (int t = 0; t < 5; t++) wp[(size_t)o * 448 + t * 80 + c] = w->data[((size_t)o * 80 + c) * 5 + t];
    CCX_TRY(fold_bn(e, "blocks.0.norm.norm", 1024, sc, sh));
    CCX_TRY(S.upload_bf16(&e->b0.W, wp)); CCX_TRY(S.upload(&e->b0.b, b->data.data(), 1024));
    CCX_TRY(S.upload(&e->b0.sc, sc)); CCX_TRY(S.upload(&e->b0.sh, sh));
  }
  for (int k = 0; k < 3; k++) {
    const std::string p = "blocks." + std::to_string(k + 1);
    CCX_TRY(load_tdnn(e, p + ".tdnn1", 1024, 1024, e->t1[k]));
    CCX_TRY(load_tdnn(e, p + ".tdnn2", 1024, 1024, e->t2[k]));
    std::vector<float> w7((size_t)ECAPA_R2_STAGES * 128 * 128 * 3), aff((size_t)ECAPA_R2_STAGES * 3 * 128), frag;
    for (int s = 0; s < ECAPA_R2_STAGES; s++) {
      const std::string q = p + ".res2net_block.blocks." + std::to_string(s);
      CCX_NEED(S, w, q + ".conv.conv.weight", 128 * 128 * 3); CCX_NEED(S, b, q + ".conv.conv.bias", 128);
      std::vector<float> sc, sh;
      CCX_TRY(fold_bn(e, q + ".norm.norm", 128, sc, sh));
      std::copy(w->data.begin(), w->data.end(), w7.begin() + (size_t)s * 128 * 128 * 3);
      for (int c = 0; c < 128; c++) { aff[(s * 3 + 0) * 128 + c] = b->data[c]; aff[(s * 3 + 1) * 128 + c] = sc[c]; aff[(s * 3 + 2) * 128 + c] = sh[c]; }
    }
    ccx_ecapa_pack_res2net(w7.data(), frag);
    CCX_TRY(S.upload_bf16(&e->r2w[k], frag)); CCX_TRY(S.upload(&e->r2aff[k], aff));
    CCX_NEED(S, w1, p + ".se_block.conv1.conv.weight", 128 * 1024); CCX_NEED(S, b1, p + ".se_block.conv1.conv.bias", 128);
    CCX_NEED(S, w2, p + ".se_block.conv2.conv.weight", 1024 * 128); CCX_NEED(S, b2, p + ".se_block.conv2.conv.bias", 1024);
    CCX_TRY(S.upload(&e->sw1[k], w1->data)); CCX_TRY(S.upload(&e->sb1[k], b1->data));
    CCX_TRY(S.upload(&e->sw2[k], w2->data)); CCX_TRY(S.upload(&e->sb2[k], b2->data));
  }
  CCX_TRY(load_tdnn(e, "mfa", 3072, 3072, e->mfa));
  {  // asp.tdnn: Conv1d(9216 -> 128) split into the part over x (a GEMM) and the part over (mean | std) (a per-crop vector)
    CCX_NEED(S, w, "asp.tdnn.conv.conv.weight", 128 * 9216); CCX_NEED(S, b, "asp.tdnn.conv.conv.bias", 128);
    std::vector<float> wx((size_t)128 * 3072), wms((size_t)128 * 6144), sc, sh;
    for (int o = 0; o < 128; o++) {
      std::copy(w->data.begin() + (size_t)o * 9216, w->data.begin() + (size_t)o * 9216 + 3072, wx.begin() + (size_t)o * 3072);
      std::copy(w->data.begin() + (size_t)o * 9216 + 3072, w->data.begin() + (size_t)(o + 1) * 9216, wms.begin() + (size_t)o * 6144);
    }
    CCX_TRY(fold_bn(e, "asp.tdnn.norm.norm", 128, sc, sh));
    CCX_TRY(S.upload_bf16(&e->Wx, wx)); CCX_TRY(S.upload(&e->wms, wms)); CCX_TRY(S.upload(&e->basp, b->data));
    CCX_TRY(S.upload(&e->asc, sc)); CCX_TRY(S.upload(&e->ash, sh));
    CCX_NEED(S, wa, "asp.conv.conv.weight", 3072 * 128); CCX_NEED(S, ba, "asp.conv.conv.bias", 3072);
    CCX_TRY(S.upload_bf16(&e->wa, wa->data)); CCX_TRY(S.upload(&e->ba, ba->data));
    std::vector<float> bsc, bsh;
    CCX_TRY(fold_bn(e, "asp_bn.norm", 6144, bsc, bsh));
    CCX_TRY(S.upload(&e->bnsc, bsc)); CCX_TRY(S.upload(&e->bnsh, bsh));
    CCX_NEED(S, wf, "fc.conv.weight", 192 * 6144); CCX_NEED(S, bf, "fc.conv.bias", 192);
    CCX_TRY(S.upload_bf16(&e->Wfc, wf->data)); CCX_TRY(S.upload(&e->bfc, bf->data));
  }
  S.staged.clear();
  // capacity: a crop of n samples has 1 + n / 160 frames and 8 halo rows
  e->Rcap = e->max_samples / ECAPA_HOP + 9L * e->max_crops;
  const size_t R = (size_t)e->Rcap + 16, C = (size_t)e->max_crops;
  CCX_TRY(S.alloc(&e->raw, R * 80, true)); CCX_TRY(S.alloc(&e->feats, R * 80 + 1024, true));
  CCX_TRY(S.alloc(&e->a0, R * 1024, true)); CCX_TRY(S.alloc(&e->u, R * 1024, true)); CCX_TRY(S.alloc(&e->v, R * 1024, true));
  CCX_TRY(S.alloc(&e->w, R * 1024, true)); CCX_TRY(S.alloc(&e->cat, R * 3072, true)); CCX_TRY(S.alloc(&e->m, R * 3072, true));
  CCX_TRY(S.alloc(&e->h32, R * 128, true)); CCX_TRY(S.alloc(&e->hid, R * 128, true));
  CCX_TRY(S.alloc(&e->gmax, C, true)); CCX_TRY(S.alloc(&e->fpart, C * ECAPA_PIECES * ECAPA_MELS, true));
  CCX_TRY(S.alloc(&e->semean, C * 1024, true)); CCX_TRY(S.alloc(&e->gates, C * 1024, true)); CCX_TRY(S.alloc(&e->stat, C * 6144, true));
  CCX_TRY(S.alloc(&e->cvec, C * 128, true)); CCX_TRY(S.alloc(&e->pooled, C * 6144 + 1024, true));
  CCX_TRY(S.alloc(&e->crop_off, C, true)); CCX_TRY(S.alloc(&e->crop_len, C, true)); CCX_TRY(S.alloc(&e->row_off, C, true)); CCX_TRY(S.alloc(&e->frames, C, true));
  e->finalized = true;
  return CCX_OK;
}

int ccx_ecapa_embed(ccx_ecapa* e, const float* wav, const int64_t* offsets, const int* n_samples, int n, float* out, void* stream_) {
  if (!e) return CCX_ERR_ARG;
  ccx_ctx* ctx = e->ctx;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, e->finalized && wav && offsets && n_samples && out && n >= 1 && n <= e->max_crops, "ecapa_embed: bad arguments (n=%d, max %d)", n, e->max_crops);
  EcapaPlan& P = e->plan_ring[e->plan_slot++ & 3];
  P.coff.resize(n); P.clen.resize(n); P.roff.resize(n); P.fr.resize(n);
  long R = 0;
  int maxT = 0;
  for (int i = 0; i < n; i++) {
    CCX_REQUIRE(ctx, n_samples[i] >= ECAPA_MIN_SAMPLES, "ecapa: crop %d (%d samples) is too short (at least %d samples)", i, n_samples[i], ECAPA_MIN_SAMPLES);
    const int T = 1 + n_samples[i] / ECAPA_HOP;
    P.coff[i] = offsets[i]; P.clen[i] = n_samples[i]; P.roff[i] = (int)R; P.fr[i] = T;
    R += T + 2 * ECAPA_HALO;
    maxT = std::max(maxT, T);
  }
  CCX_REQUIRE(ctx, R <= e->Rcap, "ecapa: %ld rows exceed capacity %ld", R, e->Rcap);
  CCX_HIP(ctx, hipMemcpyAsync(e->crop_off, P.coff.data(), n * sizeof(long), hipMemcpyHostToDevice, st));
  CCX_HIP(ctx, hipMemcpyAsync(e->crop_len, P.clen.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
  CCX_HIP(ctx, hipMemcpyAsync(e->row_off, P.roff.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
  CCX_HIP(ctx, hipMemcpyAsync(e->frames, P.fr.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
  const EcapaCrops cr{e->row_off, e->frames, n, maxT};
  const int Ri = (int)R;
  CCX_TRY(ccx_launch_ecapa_fbank(ctx, wav, e->crop_off, e->crop_len, cr, e->dft_cos, e->dft_sin, e->filt, e->raw, e->gmax, e->fpart, e->feats, st));
  {  // blocks.0: GEMM row m = feature rows m .. m + 4, the output row is their centre m + 2; rows whose window crosses a crop end land
     // in halo rows, which ecapa_halo_kernel then rewrites
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = e->feats; p.lda = 80; p.W = e->b0.W; p.ldw = 448; p.M = Ri - 4; p.N = 1024; p.K = 448; p.bias = e->b0.b;
    p.out = e->a0 + 2 * 1024; p.ldo = 1024; p.scale = e->b0.sc; p.shift = e->b0.sh; p.slope = 0.f;
    CCX_TRY(ccx_launch_gemm(ctx, EPI_BF16_LRELU_AFFINE, p, st));
    CCX_TRY(ccx_launch_ecapa_halo(ctx, e->a0, 1024, 1024, cr, st));
  }
  for (int k = 0; k < 3; k++) {
    const bf16_t* in = k == 0 ? e->a0 : e->cat + (k - 1) * 1024;
    const long ldin = k == 0 ? 1024 : 3072;
    CCX_TRY(gemm_tdnn(ctx, e->t1[k], in, ldin, Ri, 1024, 1024, e->u, 1024, st));
    CCX_TRY(ccx_launch_ecapa_res2net(ctx, e->u, 1024, e->v, 1024, cr, e->r2w[k], e->r2aff[k], k + 2, st));
    CCX_TRY(gemm_tdnn(ctx, e->t2[k], e->v, 1024, Ri, 1024, 1024, e->w, 1024, st));
    CCX_TRY(ccx_launch_ecapa_se(ctx, e->w, 1024, in, ldin, e->cat + k * 1024, 3072, cr, e->sw1[k], e->sb1[k], e->sw2[k], e->sb2[k], e->semean, e->gates, st));
  }
  CCX_TRY(gemm_tdnn(ctx, e->mfa, e->cat, 3072, Ri, 3072, 3072, e->m, 3072, st));
  CCX_TRY(ccx_launch_ecapa_ctx_stats(ctx, e->m, 3072, 3072, cr, e->stat, st));
  {
    ccx_prof_scope ps(ctx, st, "ecapa_ctx_vec_kernel", 2.0 * n * 128 * 6144, 4.0 * 128 * 6144);
    hipLaunchKernelGGL(ecapa_ctx_vec_kernel, dim3(n), dim3(256), 0, st, e->stat, e->wms, e->basp, e->cvec);
  }
  CCX_CHECK_LAUNCH(ctx);
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = e->m; p.lda = 3072; p.W = e->Wx; p.ldw = 3072; p.M = Ri; p.N = 128; p.K = 3072; p.out = e->h32; p.ldo = 128;
  CCX_TRY(ccx_launch_gemm(ctx, EPI_F32, p, st));
  {
    ccx_prof_scope ps(ctx, st, "ecapa_asp_hidden_kernel", 6.0 * R * 128, 6.0 * R * 128);
    hipLaunchKernelGGL(ecapa_asp_hidden_kernel, dim3(n, ECAPA_PIECES), dim3(256), 0, st, e->h32, e->cvec, e->asc, e->ash, e->row_off, e->frames, e->hid);
  }
  CCX_CHECK_LAUNCH(ctx);
  CCX_TRY(ccx_launch_ecapa_asp_pool(ctx, e->hid, e->m, 3072, 3072, cr, e->wa, e->ba, e->bnsc, e->bnsh, e->pooled, st));
  memset(&p, 0, sizeof(p));
  p.A = e->pooled; p.lda = 6144; p.W = e->Wfc; p.ldw = 6144; p.M = n; p.N = 192; p.K = 6144; p.bias = e->bfc; p.out = out; p.ldo = 192;
  CCX_TRY(ccx_launch_gemm(ctx, EPI_F32, p, st));
  return CCX_OK;
}

// ---------------------------------------------------------------------------------------------
// the kernels on their own (include/ccx.h: ccx_ecapa_op)
// ---------------------------------------------------------------------------------------------
#define EC_BUF(field, need)                                                                                                         \
  do {                                                                                                                              \
    CCX_REQUIRE(ctx, d->field != nullptr, "ccx_ecapa_op: %s is NULL", #field);                                                      \
    CCX_REQUIRE(ctx, ccx_aligned16(d->field), "ccx_ecapa_op: %s is not 16-byte aligned", #field);                                   \
    CCX_REQUIRE(ctx, d->field##_elems >= (int64_t)(need), "ccx_ecapa_op: %s is accessed up to element %ld, %s_elems=%ld", #field,   \
                (long)(need), #field, (long)d->field##_elems);                                                                      \
  } while (0)
#define EC_PARAM(field, efield, count)                                                                                              \
  do {                                                                                                                              \
    CCX_REQUIRE(ctx, d->field != nullptr, "ccx_ecapa_op: %s is NULL", #field);                                                      \
    CCX_REQUIRE(ctx, ccx_aligned16(d->field), "ccx_ecapa_op: %s is not 16-byte aligned", #field);                                   \
    CCX_REQUIRE(ctx, d->efield == (int64_t)(count), "ccx_ecapa_op: %s holds %ld elements (%s), the kernel reads %ld", #field,       \
                (long)d->efield, #efield, (long)(count));                                                                           \
  } while (0)
#define EC_LD(field, live)                                                                                                          \
  CCX_REQUIRE(ctx, d->field >= (live) && d->field % 8 == 0 && d->field <= (1 << 20), "ccx_ecapa_op: %s = %ld must be a multiple of 8 in [%d, 2^20]", \
              #field, (long)d->field, (int)(live))
#define EC_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

int ccx_ecapa_op(ccx_ctx* ctx, int op, const ccx_ecapa_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_ecapa_op: desc is NULL");
  CCX_REQUIRE(ctx, op >= CCX_ECAPA_FBANK && op <= CCX_ECAPA_ASP_POOL, "ccx_ecapa_op: unknown op %d", op);
  CCX_REQUIRE(ctx, d->rows >= 1 && d->rows <= (1 << 24), "ccx_ecapa_op: rows = %d out of range [1, 2^24]", d->rows);
  CCX_REQUIRE(ctx, d->n >= 1 && d->n <= 65535, "ccx_ecapa_op: n = %d out of range [1, 65535]", d->n);
  CCX_REQUIRE(ctx, d->row_off && d->frames, "ccx_ecapa_op: row_off or frames is NULL");
  int maxT = 0;
  {
    std::vector<std::pair<int, int>> iv(d->n);
    for (int i = 0; i < d->n; i++) {
      const int r = d->row_off[i], T = d->frames[i];
      CCX_REQUIRE(ctx, T >= ECAPA_MIN_FRAMES, "ccx_ecapa_op: frames[%d] = %d, a crop needs at least %d frames (the reflection halo)", i, T, ECAPA_MIN_FRAMES);
      CCX_REQUIRE(ctx, r >= 0 && r <= d->rows && T + 2 * ECAPA_HALO <= d->rows - r, "ccx_ecapa_op: row_off[%d] = %d, frames[%d] = %d (+ 8 halo rows) leave the %d rows", i, r, i, T, d->rows);
      iv[i] = {r, i};
      maxT = std::max(maxT, T);
    }
    std::sort(iv.begin(), iv.end());
    for (int i = 1; i < d->n; i++) {
      const int a = iv[i - 1].second, b = iv[i].second;
      CCX_REQUIRE(ctx, d->row_off[a] + d->frames[a] + 2 * ECAPA_HALO <= d->row_off[b], "ccx_ecapa_op: row_off / frames: crops %d and %d overlap", a, b);
    }
  }
  const int64_t rows = d->rows;
  switch (op) {
    case CCX_ECAPA_FBANK:
      CCX_REQUIRE(ctx, d->offsets && d->n_samples, "ccx_ecapa_op: offsets or n_samples is NULL");
      CCX_REQUIRE(ctx, d->wav != nullptr && ((uintptr_t)d->wav & 3) == 0, "ccx_ecapa_op: wav is NULL or not 4-byte aligned");
      for (int i = 0; i < d->n; i++) {
        CCX_REQUIRE(ctx, d->n_samples[i] >= ECAPA_MIN_SAMPLES, "ccx_ecapa_op: n_samples[%d] = %d, a crop needs at least %d samples", i, d->n_samples[i], ECAPA_MIN_SAMPLES);
        CCX_REQUIRE(ctx, d->offsets[i] >= 0 && d->offsets[i] + d->n_samples[i] <= d->wav_elems, "ccx_ecapa_op: offsets[%d] = %ld with n_samples[%d] = %d leaves wav_elems = %ld", i, (long)d->offsets[i], i, d->n_samples[i], (long)d->wav_elems);
        CCX_REQUIRE(ctx, d->frames[i] == 1 + d->n_samples[i] / ECAPA_HOP, "ccx_ecapa_op: frames[%d] = %d, n_samples[%d] = %d gives %d", i, d->frames[i], i, d->n_samples[i], 1 + d->n_samples[i] / ECAPA_HOP);
      }
      EC_PARAM(window, window_elems, ECAPA_NFFT); EC_PARAM(filters, filters_elems, ECAPA_MELS * ECAPA_BINS);
      EC_BUF(feats, rows * ECAPA_MELS);
      break;
    case CCX_ECAPA_RES2NET:
      CCX_REQUIRE(ctx, d->dilation >= 1 && d->dilation <= 4, "ccx_ecapa_op: dilation = %d out of range [1, 4]", d->dilation);
      CCX_REQUIRE(ctx, d->w_host && d->aff_host, "ccx_ecapa_op: w_host or aff_host is NULL");
      EC_LD(ldx, 1024); EC_LD(ldy, 1024);
      EC_BUF(x, (rows - 1) * d->ldx + 1024); EC_BUF(y, (rows - 1) * d->ldy + 1024);
      CCX_REQUIRE(ctx, d->x != d->y, "ccx_ecapa_op: y aliases x");
      break;
    case CCX_ECAPA_SE:
      EC_LD(ldx, 1024); EC_LD(ldy, 1024); EC_LD(ld_resid, 1024);
      EC_BUF(x, (rows - 1) * d->ldx + 1024); EC_BUF(y, (rows - 1) * d->ldy + 1024); EC_BUF(resid, (rows - 1) * d->ld_resid + 1024);
      EC_PARAM(w1, w1_elems, 128 * 1024); EC_PARAM(b1, b1_elems, 128); EC_PARAM(w2, w2_elems, 1024 * 128); EC_PARAM(b2, b2_elems, 1024);
      if (d->gates) EC_BUF(gates, (int64_t)d->n * 1024);
      break;
    default:
      CCX_REQUIRE(ctx, d->channels >= 64 && d->channels <= 8192 && d->channels % 64 == 0, "ccx_ecapa_op: channels = %d must be a multiple of 64 in [64, 8192]", d->channels);
      EC_LD(ldx, d->channels);
      EC_BUF(x, (rows - 1) * d->ldx + d->channels); EC_BUF(hidden, rows * 128);
      EC_PARAM(wa, wa_elems, (int64_t)d->channels * 128); EC_PARAM(ba, ba_elems, d->channels);
      EC_PARAM(bn_scale, bn_elems, 2 * d->channels); EC_PARAM(bn_shift, bn_elems, 2 * d->channels);
      EC_BUF(pooled, (int64_t)d->n * 2 * d->channels);
  }

  ccx_op_scratch sc;
  int *d_off = nullptr, *d_fr = nullptr;
  EC_HIP(sc.upload(&d_off, d->row_off, (size_t)d->n));
  EC_HIP(sc.upload(&d_fr, d->frames, (size_t)d->n));
  const EcapaCrops cr{d_off, d_fr, d->n, maxT};
  int rc = CCX_OK;
  switch (op) {
    case CCX_ECAPA_FBANK: {
      std::vector<float> win(ECAPA_NFFT), fb((size_t)ECAPA_MELS * ECAPA_BINS), dc, ds, fl;
      EC_HIP(hipMemcpy(win.data(), d->window, win.size() * 4, hipMemcpyDeviceToHost));
      EC_HIP(hipMemcpy(fb.data(), d->filters, fb.size() * 4, hipMemcpyDeviceToHost));
      ccx_ecapa_fbank_tables(win.data(), fb.data(), dc, ds, fl);
      std::vector<long> co(d->n);
      for (int i = 0; i < d->n; i++) co[i] = d->offsets[i];
      float *t_c = nullptr, *t_s = nullptr, *t_f = nullptr, *raw = nullptr, *part = nullptr;
      unsigned int* gmax = nullptr;
      long* d_co = nullptr; int* d_len = nullptr;
      EC_HIP(sc.upload(&t_c, dc.data(), dc.size())); EC_HIP(sc.upload(&t_s, ds.data(), ds.size())); EC_HIP(sc.upload(&t_f, fl.data(), fl.size()));
      EC_HIP(sc.upload(&d_co, co.data(), co.size())); EC_HIP(sc.upload(&d_len, d->n_samples, (size_t)d->n));
      EC_HIP(sc.alloc(&raw, (size_t)rows * ECAPA_MELS)); EC_HIP(sc.alloc(&part, (size_t)d->n * ECAPA_PIECES * ECAPA_MELS)); EC_HIP(sc.alloc(&gmax, (size_t)d->n));
      rc = ccx_launch_ecapa_fbank(ctx, (const float*)d->wav, d_co, d_len, cr, t_c, t_s, t_f, raw, gmax, part, (bf16_t*)d->feats, st);
      break;
    }
    case CCX_ECAPA_RES2NET: {
      std::vector<float> frag;
      ccx_ecapa_pack_res2net(d->w_host, frag);
      std::vector<bf16_t> fb(frag.size());
      for (size_t i = 0; i < frag.size(); i++) fb[i] = ccx_host_f32_to_bf16(frag[i]);
      bf16_t* d_w = nullptr; float* d_aff = nullptr;
      EC_HIP(sc.upload(&d_w, fb.data(), fb.size())); EC_HIP(sc.upload(&d_aff, d->aff_host, (size_t)ECAPA_R2_STAGES * 3 * 128));
      rc = ccx_launch_ecapa_res2net(ctx, (const bf16_t*)d->x, d->ldx, (bf16_t*)d->y, d->ldy, cr, d_w, d_aff, d->dilation, st);
      break;
    }
    case CCX_ECAPA_SE: {
      float *mean = nullptr, *gates = (float*)d->gates;
      EC_HIP(sc.alloc(&mean, (size_t)d->n * 1024));
      if (!gates) EC_HIP(sc.alloc(&gates, (size_t)d->n * 1024));
      rc = ccx_launch_ecapa_se(ctx, (const bf16_t*)d->x, d->ldx, (const bf16_t*)d->resid, d->ld_resid, (bf16_t*)d->y, d->ldy, cr, (const float*)d->w1,
                               (const float*)d->b1, (const float*)d->w2, (const float*)d->b2, mean, gates, st);
      break;
    }
    default:
      rc = ccx_launch_ecapa_asp_pool(ctx, (const bf16_t*)d->hidden, (const bf16_t*)d->x, d->ldx, d->channels, cr, (const bf16_t*)d->wa,
                                     (const float*)d->ba, (const float*)d->bn_scale, (const float*)d->bn_shift, (bf16_t*)d->pooled, st);
  }
  EC_HIP(hipStreamSynchronize(st));      // the scratch is freed on return
  return rc;
}

}  // extern "C"

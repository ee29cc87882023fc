// dualpath.hip -- dual-path SepFormer separator of libccx (SpeechBrain's Dual_Path_Model with SBTransformerBlock intra / inter
// models: the published sepformer-* checkpoints).  Semantics follow SpeechBrain from recollection [UPSTREAM-RECALL], parity
// unpinned; the fp64 restatement is tests/dualpath_reference.py.
//
// Data layout: ONE token buffer of rows [utterance][chunk s][position k][256] that is never permuted.  LayerNorm, every GEMM and the
// FFN are row-wise; an intra-chunk sequence is K contiguous rows, an inter-chunk sequence S rows at stride K: only the attention
// kernel (a table of first row, row stride, length) and the positional-encoding add know which is which.  Every linear layer runs on
// the shared bf16 MFMA GEMM (gemm_bf16.hip); the kernels here are what that family cannot express.  Correctness first: no fused
// layer kernel, nothing tuned.
#include <math.h>
#include <algorithm>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "dualpath.h"
#include "elementwise.h"
#include "gemm_bf16.h"
#include "model_store.h"
#include "op_scratch.h"
#include "sb_softmax.h"
#include "sb_stack.h"

namespace {

constexpr int D = CCX_DP_D;

// ---------------------------------------------------------------------------------------------------------------------------------
// Attention, head_dim 32, 8 heads, non-causal, sequences given by (first row, row stride, length).  One wave per (sequence, head,
// 16-query tile); a block is four heads.  S^T = K Q^T with ONE v_mfma_f32_16x16x32_bf16 per 16-key tile (the whole head in one
// K-step), so a lane owns one query column and four keys of it; those accumulator registers are, unchanged, the A operand of
// O = P V (v_mfma_f32_16x16x16_bf16: row = query, k = key), two of them for the 32 output columns.  Online softmax over blocks of
// CCX_DP_KEY_BLOCK keys: the step and its rounding rule are sb_softmax.h, shared with sep_attention_kernel; q, k, v arrive as bf16.
// Rows past a sequence's length are never read: loads clamp to its last row, those keys score -inf, those queries are not stored.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dp_attention_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ seq,
                                                           bf16_t* __restrict__ out, float scale_log2e) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sq = blockIdx.x, head = blockIdx.y * 4 + wave, qt = blockIdx.z;
  const int first = seq[3 * sq], stride = seq[3 * sq + 1], len = seq[3 * sq + 2];
  if (qt * 16 >= len) return;                                     // block-uniform
  const int l15 = lane & 15, h4 = lane >> 4;
  const int n_kt = (len + 15) >> 4;
  auto row_of = [&](int i) -> long { return (long)first + (long)(i < len ? i : len - 1) * stride; };
  const bf16_t* base = qkv + head * 32;
  // B operand of S^T = K Q^T: B[k = d = 8 h4 + j][col = query l15]
  const bf16x8 qf = *(const bf16x8*)(base + row_of(qt * 16 + l15) * (3 * D) + 8 * h4);
  float m_run = -1e30f, l_run = 0.f;
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;                        // O tiles: col = d (l15 / 16 + l15), rows = query 4 h4 + r
  constexpr int NT = CCX_DP_KEY_BLOCK / 16;
  for (int kt0 = 0; kt0 < n_kt; kt0 += NT) {
    const int nk = (n_kt - kt0) < NT ? (n_kt - kt0) : NT;
    f32x4 s[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
      if (t < nk) {
        // A operand: K[key l15][d = 8 h4 + j]
        const bf16x8 kf = *(const bf16x8*)(base + D + row_of((kt0 + t) * 16 + l15) * (3 * D) + 8 * h4);
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        // s[t][r] = score(query l15, key (kt0 + t) 16 + 4 h4 + r)
      }
    const float alpha = nk == NT ? sb_online_step<NT, true>(s, nk, kt0 * 16, len, h4, scale_log2e, m_run, l_run)
                                 : sb_online_step<NT, false>(s, nk, kt0 * 16, len, h4, scale_log2e, m_run, l_run);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float a = sb_row_value(alpha, h4, r);
      o0[r] *= a;
      o1[r] *= a;
    }
#pragma unroll
    for (int t = 0; t < NT; t++)
      if (t < nk) {
        const bf16x4v pa = sb_pack_p(s[t]);                          // A operand: P[query l15][key 4 h4 + j]
        bf16x4v v0, v1;                                              // B operand: V[key 4 h4 + j][d = l15 (+ 16)]
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const bf16_t* vr = base + 2 * D + row_of((kt0 + t) * 16 + 4 * h4 + j) * (3 * D);
          v0[j] = (short)vr[l15];
          v1[j] = (short)vr[16 + l15];
        }
        o0 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa, v0, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa, v1, o1, 0, 0, 0);
      }
  }
  const float lt = sb_query_sum(l_run);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int q = qt * 16 + 4 * h4 + r;
    const float inv = 1.0f / sb_row_value(lt, h4, r);
    if (q < len) {
      bf16_t* o = out + ((long)first + (long)q * stride) * D + head * 32;
      o[l15] = f32_to_bf16(o0[r] * inv);
      o[16 + l15] = f32_to_bf16(o1[r] * inv);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// GroupNorm(1, 256, eps 1e-8) of an utterance: statistics over ALL its rows x 256 channels, in fp32, two passes -- the second sums
// (x - mean)^2, not E[x^2] - mean^2.  An utterance's rows are cut into CCX_DP_GN_PARTS slices, one block each; the partial sums meet in
// a fixed order (no atomics: repeats are bit-identical).  tab [n_utt][2]: first row, rows.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dp_block_sum(float v, float* red) {       // 256 threads; every thread gets the sum
  v = wave_reduce_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float dp_parts_sum(const float* __restrict__ p) {
  float s = 0.f;
  for (int i = 0; i < CCX_DP_GN_PARTS; i++) s += p[i];
  return s;
}

// pass 0: part[u][b] = sum of the slice; pass 1: part[n_utt .. ][u][b] = sum of (x - mean)^2 of the slice
__global__ __launch_bounds__(256) void dp_gn_stats_kernel(const float* __restrict__ x, const int* __restrict__ tab, float* __restrict__ part,
                                                          int n_utt, int pass) {
  __shared__ float red[4];
  const int u = blockIdx.y, b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = tab[2 * u], nrows = tab[2 * u + 1];
  const int per = ccx_cdiv(nrows, CCX_DP_GN_PARTS);
  const int r0 = b * per, r1 = (r0 + per) < nrows ? (r0 + per) : nrows;
  float mean = 0.f;
  if (pass == 1) mean = dp_parts_sum(part + (long)u * CCX_DP_GN_PARTS) / ((float)nrows * (float)D);
  float acc = 0.f;
  for (int r = r0 + wave; r < r1; r += 4) {
    const float4 v = ((const float4*)(x + (long)(row0 + r) * D))[lane];
    if (pass == 0) acc += (v.x + v.y) + (v.z + v.w);
    else {
      const float a = v.x - mean, c = v.y - mean, d = v.z - mean, e = v.w - mean;
      acc += (a * a + c * c) + (d * d + e * e);
    }
  }
  acc = dp_block_sum(acc, red);
  if (threadIdx.x == 0) part[((long)pass * n_utt + u) * CCX_DP_GN_PARTS + b] = acc;
}

template <bool BF16_OUT>
__global__ __launch_bounds__(256) void dp_gn_apply_kernel(const float* __restrict__ x, const int* __restrict__ tab, const float* __restrict__ part,
                                                          int n_utt, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* skip, float* out_f32, bf16_t* __restrict__ out_bf16) {
  const int u = blockIdx.y, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row0 = tab[2 * u], nrows = tab[2 * u + 1];
  if (r >= nrows) return;
  const float n = (float)nrows * (float)D;
  const float mean = dp_parts_sum(part + (long)u * CCX_DP_GN_PARTS) / n;
  const float rstd = 1.0f / sqrtf(dp_parts_sum(part + ((long)n_utt + u) * CCX_DP_GN_PARTS) / n + 1e-8f);
  const long i = (long)(row0 + r) * (D / 4) + lane;
  const float4 v = ((const float4*)x)[i], g = ((const float4*)gamma)[lane], b = ((const float4*)beta)[lane];
  float4 y = make_float4(g.x * (v.x - mean) * rstd + b.x, g.y * (v.y - mean) * rstd + b.y, g.z * (v.z - mean) * rstd + b.z,
                         g.w * (v.w - mean) * rstd + b.w);
  if constexpr (BF16_OUT) {
    uint2 o;
    o.x = pack_bf16x2(y.x, y.y);
    o.y = pack_bf16x2(y.z, y.w);
    ((uint2*)out_bf16)[i] = o;
  } else {
    const float4 k = ((const float4*)skip)[i];
    ((float4*)out_f32)[i] = make_float4(y.x + k.x, y.y + k.y, y.z + k.z, y.w + k.w);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Segmentation, positional encoding and overlap-add: gathers over the utterance table.  The padded signal of an utterance is
// [P zeros | L frames | gap zeros | P zeros] with P = K / 2; chunk s is its positions s P .. s P + K - 1.  One wave per row.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dp_segment_kernel(const float* __restrict__ frames, const ccx_dp_utt* __restrict__ utt, int K,
                                                         float* __restrict__ tok) {
  const ccx_dp_utt U = utt[blockIdx.y];
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= U.S * K) return;
  const int s = r / K, k = r - s * K;
  const int l = s * (K / 2) + k - K / 2;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                      // padding is written as zeros on every call
  if (l >= 0 && l < U.L) v = ((const float4*)(frames + (long)(U.frame0 + l) * D))[lane];
  ((float4*)(tok + (long)(U.tok0 + r) * D))[lane] = v;
}

__global__ __launch_bounds__(256) void dp_pe_add_kernel(const float* __restrict__ x, const ccx_dp_utt* __restrict__ utt, int K, int axis,
                                                        const float* __restrict__ pe, float* __restrict__ out) {
  const ccx_dp_utt U = utt[blockIdx.y];
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= U.S * K) return;
  const int s = r / K, k = r - s * K;
  const long i = (long)(U.tok0 + r) * (D / 4) + lane;
  const float4 v = ((const float4*)x)[i], p = ((const float4*)(pe + (long)(axis ? s : k) * D))[lane];
  ((float4*)out)[i] = make_float4(v.x + p.x, v.y + p.y, v.z + p.z, v.w + p.w);
}

// frame l sits at padded position p = l + P: entry p % P of chunk p / P and entry p % P + P of the chunk before it -- exactly two,
// both inside the utterance's S chunks (gap >= 1), so the sum is a gather
__global__ __launch_bounds__(256) void dp_overlap_add_kernel(const float* __restrict__ fc, const ccx_dp_utt* __restrict__ utt, int K, int n_spk,
                                                             bf16_t* __restrict__ out) {
  const ccx_dp_utt U = utt[blockIdx.y];
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= U.L * n_spk) return;
  const int l = i / n_spk, s = i - l * n_spk, P = K / 2;
  const int j1 = (l + P) / P, k1 = (l + P) - j1 * P;
  const long ra = (long)U.tok0 + (long)j1 * K + k1, rb = (long)U.tok0 + (long)(j1 - 1) * K + k1 + P;
  const float4 a = ((const float4*)(fc + (ra * n_spk + s) * D))[lane], b = ((const float4*)(fc + (rb * n_spk + s) * D))[lane];
  uint2 o;
  o.x = pack_bf16x2(a.x + b.x, a.y + b.y);
  o.y = pack_bf16x2(a.z + b.z, a.w + b.w);
  ((uint2*)(out + ((long)(U.frame0 + l) * n_spk + s) * D))[lane] = o;
}

__device__ __forceinline__ float dp_gate1(float a, float b) { return tanhf(a) * (1.0f / (1.0f + expf(-b))); }

__global__ void dp_gate_kernel(const float* __restrict__ g, bf16_t* __restrict__ out, long n4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // float4 index of the output
  if (i >= n4) return;
  const long r = i >> 6, c4 = i & 63;
  const float4 a = ((const float4*)(g + r * 2 * D))[c4], b = ((const float4*)(g + r * 2 * D + D))[c4];
  uint2 o;
  o.x = pack_bf16x2(dp_gate1(a.x, b.x), dp_gate1(a.y, b.y));
  o.y = pack_bf16x2(dp_gate1(a.z, b.z), dp_gate1(a.w, b.w));
  ((uint2*)out)[i] = o;
}

// Encoder: Conv1d(1 -> 256, kernel, stride kernel / 2, no bias) + ReLU, frame-major.  One wave per frame, four filters per lane.
__global__ __launch_bounds__(256) void dp_encoder_kernel(const float* __restrict__ mix, long mix_stride, const ccx_dp_utt* __restrict__ utt,
                                                         int kernel, const float* __restrict__ w, float* __restrict__ frames) {
  const ccx_dp_utt U = utt[blockIdx.y];
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (l >= U.L) return;
  const float* x = mix + (long)blockIdx.y * mix_stride + (long)(kernel / 2) * l;   // (kernel / 2) l + kernel <= T by the rule of L
  const float* wr = w + (long)(4 * lane) * kernel;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int k = 0; k < kernel; k++) {
    const float xv = x[k];
    a0 = fmaf(wr[k], xv, a0);
    a1 = fmaf(wr[kernel + k], xv, a1);
    a2 = fmaf(wr[2 * kernel + k], xv, a2);
    a3 = fmaf(wr[3 * kernel + k], xv, a3);
  }
  ((float4*)(frames + (long)(U.frame0 + l) * D))[lane] = make_float4(fmaxf(a0, 0.f), fmaxf(a1, 0.f), fmaxf(a2, 0.f), fmaxf(a3, 0.f));
}

// Mask (ReLU) * encoder output, ConvTranspose1d(256 -> 1, kernel, stride = kernel / 2), pad / trim to T, for NSPK sources.  One wave per
// group of `stride` output samples t = stride l + k: they need exactly the frames l (taps k) and l - 1 (taps k + stride).  Lanes split
// the 256 channels; the group's stride NSPK results leave as one float per lane (lane = k NSPK + s; stride NSPK <= 48).
template <int NSPK>
__global__ __launch_bounds__(256) void dp_decoder_kernel(const float* __restrict__ feats, const float* __restrict__ mask,
                                                         const ccx_dp_utt* __restrict__ utt, int kernel, const float* __restrict__ wdec,
                                                         float* __restrict__ out, long out_stride) {
  const ccx_dp_utt U = utt[blockIdx.y];
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int stride = kernel / 2;
  const long t0 = (long)stride * l;
  if (t0 >= out_stride) return;
  float g[2][NSPK][4];
#pragma unroll
  for (int dl = 0; dl < 2; dl++) {
    const int ll = l - dl;
    const bool ok = ll >= 0 && ll < U.L;
    const long fr = U.frame0 + (ok ? ll : 0);
    const float4 f = ((const float4*)(feats + fr * D))[lane];
#pragma unroll
    for (int s = 0; s < NSPK; s++) {
      const float4 m = ((const float4*)(mask + (fr * NSPK + s) * D))[lane];
      g[dl][s][0] = ok ? f.x * fmaxf(m.x, 0.f) : 0.f;
      g[dl][s][1] = ok ? f.y * fmaxf(m.y, 0.f) : 0.f;
      g[dl][s][2] = ok ? f.z * fmaxf(m.z, 0.f) : 0.f;
      g[dl][s][3] = ok ? f.w * fmaxf(m.w, 0.f) : 0.f;
    }
  }
  const float* wr = wdec + (long)(4 * lane) * kernel;
  float res = 0.f;
  for (int k = 0; k < stride; k++) {
    float w0[4], w1[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      w0[j] = wr[j * kernel + k];
      w1[j] = wr[j * kernel + k + stride];
    }
#pragma unroll
    for (int s = 0; s < NSPK; s++) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 4; j++) a += g[0][s][j] * w0[j] + g[1][s][j] * w1[j];
      a = wave_reduce_sum(a);
      if (lane == k * NSPK + s) res = a;
    }
  }
  const long t = t0 + lane / NSPK;
  if (lane < stride * NSPK && t < out_stride) out[((long)blockIdx.y * out_stride + t0) * NSPK + lane] = t < U.T ? res : 0.f;
}

}  // namespace

// ---- the launchers of dualpath.h ----
static constexpr float kDpScaleLog2e = 0.17677669529663689f * 1.4426950408889634f;   // 1 / sqrt(32)

int ccx_launch_dp_attention(ccx_ctx* ctx, const bf16_t* qkv, const int* seq, int n_seq, int max_len, bf16_t* out, hipStream_t st) {
  {
    ccx_prof_scope ps(ctx, st, "dp_attention_kernel", 4.0 * n_seq * (double)max_len * max_len * D, 0.0);
    hipLaunchKernelGGL(dp_attention_kernel, dim3(n_seq, 2, ccx_cdiv(max_len, 16)), dim3(256), 0, st, qkv, seq, out, kDpScaleLog2e);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dp_group_norm(ccx_ctx* ctx, const float* x, const int* tab, int n_utt, int max_rows, const float* gamma, const float* beta,
                             const float* skip, float* out_f32, bf16_t* out_bf16, float* part, hipStream_t st) {
  {
    ccx_prof_scope ps(ctx, st, "dp_group_norm", 0.0, 0.0);
    hipLaunchKernelGGL(dp_gn_stats_kernel, dim3(CCX_DP_GN_PARTS, n_utt), dim3(256), 0, st, x, tab, part, n_utt, 0);
    hipLaunchKernelGGL(dp_gn_stats_kernel, dim3(CCX_DP_GN_PARTS, n_utt), dim3(256), 0, st, x, tab, part, n_utt, 1);
    const dim3 grid(ccx_cdiv(max_rows, 4), n_utt);
    if (out_bf16) {
      hipLaunchKernelGGL(dp_gn_apply_kernel<true>, grid, dim3(256), 0, st, x, tab, part, n_utt, gamma, beta, skip, out_f32, out_bf16);
    } else {
      hipLaunchKernelGGL(dp_gn_apply_kernel<false>, grid, dim3(256), 0, st, x, tab, part, n_utt, gamma, beta, skip, out_f32, out_bf16);
    }
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dp_segment(ccx_ctx* ctx, const float* frames, const ccx_dp_utt* utt, int n_utt, int K, int max_S, float* tok, hipStream_t st) {
  {
    ccx_prof_scope ps(ctx, st, "dp_segment_kernel", 0.0, 0.0);
    hipLaunchKernelGGL(dp_segment_kernel, dim3(ccx_cdiv(max_S * K, 4), n_utt), dim3(256), 0, st, frames, utt, K, tok);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dp_overlap_add(ccx_ctx* ctx, const float* fc, const ccx_dp_utt* utt, int n_utt, int K, int max_L, int n_spk, bf16_t* out,
                              hipStream_t st) {
  {
    ccx_prof_scope ps(ctx, st, "dp_overlap_add_kernel", 0.0, 0.0);
    hipLaunchKernelGGL(dp_overlap_add_kernel, dim3(ccx_cdiv(max_L * n_spk, 4), n_utt), dim3(256), 0, st, fc, utt, K, n_spk, out);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dp_pe_add(ccx_ctx* ctx, const float* x, const ccx_dp_utt* utt, int n_utt, int K, int max_S, int axis, const float* pe,
                         float* out, hipStream_t st) {
  {
    ccx_prof_scope ps(ctx, st, "dp_pe_add_kernel", 0.0, 0.0);
    hipLaunchKernelGGL(dp_pe_add_kernel, dim3(ccx_cdiv(max_S * K, 4), n_utt), dim3(256), 0, st, x, utt, K, axis, pe, out);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dp_gate(ccx_ctx* ctx, const float* g, bf16_t* out, long rows, hipStream_t st) {
  const long n4 = rows * (D / 4);
  {
    ccx_prof_scope ps(ctx, st, "dp_gate_kernel", 0.0, 0.0);
    hipLaunchKernelGGL(dp_gate_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, g, out, n4);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dp_encoder(ccx_ctx* ctx, const float* mix, long mix_stride, const ccx_dp_utt* utt, int n_utt, int max_L, int kernel,
                          const float* w, float* frames, hipStream_t st) {
  {
    ccx_prof_scope ps(ctx, st, "dp_encoder_kernel", 0.0, 0.0);
    hipLaunchKernelGGL(dp_encoder_kernel, dim3(ccx_cdiv(max_L, 4), n_utt), dim3(256), 0, st, mix, mix_stride, utt, kernel, w, frames);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dp_decoder(ccx_ctx* ctx, const float* feats, const float* mask, const ccx_dp_utt* utt, int n_utt, int kernel, int n_spk,
                          const float* wdec, float* out, long out_stride, hipStream_t st) {
  const dim3 grid(ccx_cdiv((int)((out_stride + kernel / 2 - 1) / (kernel / 2)), 4), n_utt);
  ccx_prof_scope ps(ctx, st, "dp_decoder_kernel", 0.0, 0.0);
#define DP_DEC(NS)                                                                                                          \
  case NS:                                                                                                                  \
    hipLaunchKernelGGL(dp_decoder_kernel<NS>, grid, dim3(256), 0, st, feats, mask, utt, kernel, wdec, out, out_stride);      \
    break
  switch (n_spk) {
    DP_DEC(1); DP_DEC(2); DP_DEC(3);
    default: return ccx_fail(ctx, CCX_ERR_ARG, "dp_decoder: n_spk = %d, built for 1 to 3 sources", n_spk);
  }
#undef DP_DEC
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the model handle
// ---------------------------------------------------------------------------------------------------------------------------------
struct ccx_dualpath {
  ccx_ctx* ctx = nullptr;
  ccx_dualpath_dims d{};
  int max_tokens = 0, max_utts = 0, pe_len = 0;
  bool finalized = false;
  ccx_dev_store store{"dualpath"};
  float *w_enc = nullptr, *w_dec = nullptr, *gn0_g = nullptr, *gn0_b = nullptr, *prelu = nullptr, *b_fc = nullptr, *b_og = nullptr, *pe = nullptr;
  bf16_t *W_in = nullptr, *W_fc = nullptr, *W_og = nullptr, *W_end = nullptr;
  std::vector<SbStack> intra, inter;
  // workspaces: frame buffers [frames][256], token buffers [tokens][.]
  float *feats = nullptr, *xf = nullptr, *x = nullptr, *h = nullptr, *y = nullptr, *fc = nullptr, *g2 = nullptr, *mk = nullptr, *part = nullptr;
  bf16_t *xn = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr, *ya = nullptr, *yb = nullptr;
  ccx_dp_utt* utt = nullptr;
  int *seq_intra = nullptr, *seq_inter = nullptr, *gn_tok = nullptr, *gn_frame = nullptr;
};

namespace {

int dp_check_dims(ccx_ctx* ctx, const ccx_dualpath_dims& d) {
  CCX_REQUIRE(ctx, d.n_filters == D, "dualpath: n_filters = %d, the kernels are built for 256", d.n_filters);
  CCX_REQUIRE(ctx, d.d_model == D, "dualpath: d_model = %d, the kernels are built for 256", d.d_model);
  CCX_REQUIRE(ctx, d.n_head == 8, "dualpath: n_head = %d, the attention kernel is built for 8 heads of 32", d.n_head);
  CCX_REQUIRE(ctx, d.kernel >= 2 && d.kernel <= 32 && d.kernel % 2 == 0, "dualpath: kernel = %d must be even and in [2, 32]", d.kernel);
  CCX_REQUIRE(ctx, d.stride == d.kernel / 2, "dualpath: stride = %d must be kernel / 2 = %d", d.stride, d.kernel / 2);
  CCX_REQUIRE(ctx, d.segment >= 2 && d.segment <= 256 && d.segment % 2 == 0, "dualpath: segment = %d must be even and in [2, 256]", d.segment);
  CCX_REQUIRE(ctx, d.d_ffn >= 64 && d.d_ffn <= 2048 && d.d_ffn % 64 == 0, "dualpath: d_ffn = %d must be a multiple of 64 in [64, 2048]", d.d_ffn);
  CCX_REQUIRE(ctx, d.n_layers >= 1 && d.n_layers <= 8, "dualpath: n_layers = %d out of range [1, 8]", d.n_layers);
  CCX_REQUIRE(ctx, d.n_blocks >= 1 && d.n_blocks <= 8, "dualpath: n_blocks = %d out of range [1, 8]", d.n_blocks);
  CCX_REQUIRE(ctx, d.n_spk >= 1 && d.n_spk <= 3, "dualpath: n_spk = %d out of range [1, 3]", d.n_spk);
  return CCX_OK;
}

int dp_gemm(ccx_ctx* ctx, int epi, const bf16_t* A, const bf16_t* W, int M, int N, int K, const float* bias, void* out, const float* resid,
            hipStream_t st) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.lda = K; p.W = W; p.ldw = K; p.M = M; p.N = N; p.K = K; p.bias = bias; p.out = out; p.ldo = N; p.resid = resid; p.ldr = N;
  return ccx_launch_gemm(ctx, epi, p, st);
}

// x += GroupNorm(transformer(x + pe)) over the sequences of `seq`: one SBTransformerBlock + the norm and skip of a dual block half
int dp_run_transformer(ccx_dualpath* s, const SbStack& B, const int* seq, int n_seq, int max_len, int axis, int n_tok, int n_utt,
                       int max_S, hipStream_t st) {
  ccx_ctx* ctx = s->ctx;
  const int F = s->d.d_ffn, K = s->d.segment;
  CCX_TRY(ccx_launch_dp_pe_add(ctx, s->x, s->utt, n_utt, K, max_S, axis, s->pe, s->h, st));
  for (const SbLayer& L : B.layers) {
    CCX_TRY(ccx_launch_layernorm(ctx, s->h, D, L.ln1_g, L.ln1_b, s->xn, nullptr, D, n_tok, D, 1e-6f, st));
    CCX_TRY(dp_gemm(ctx, EPI_BF16, s->xn, L.Wqkv, n_tok, 3 * D, D, L.bqkv, s->qkv, nullptr, st));
    CCX_TRY(ccx_launch_dp_attention(ctx, s->qkv, seq, n_seq, max_len, s->att, st));
    CCX_TRY(dp_gemm(ctx, EPI_F32_RESID, s->att, L.Wo, n_tok, D, D, L.bo, s->h, s->h, st));
    CCX_TRY(ccx_launch_layernorm(ctx, s->h, D, L.ln2_g, L.ln2_b, s->xn, nullptr, D, n_tok, D, 1e-6f, st));
    CCX_TRY(dp_gemm(ctx, EPI_BF16_RELU, s->xn, L.W1, n_tok, F, D, L.b1, s->hid, nullptr, st));
    CCX_TRY(dp_gemm(ctx, EPI_F32_RESID, s->hid, L.W2, n_tok, D, F, L.b2, s->h, s->h, st));
  }
  CCX_TRY(ccx_launch_layernorm(ctx, s->h, D, B.lnf_g, B.lnf_b, nullptr, s->y, D, n_tok, D, 1e-6f, st));
  return ccx_launch_dp_group_norm(ctx, s->y, s->gn_tok, n_utt, max_S * K, B.norm_g, B.norm_b, s->x, s->x, nullptr, s->part, st);
}

}  // namespace

extern "C" {

int ccx_dualpath_create(ccx_ctx* ctx, const ccx_dualpath_dims* dims, int max_tokens, int max_utts, ccx_dualpath** out) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, dims && out, "ccx_dualpath_create: null argument");
  CCX_TRY(dp_check_dims(ctx, *dims));
  CCX_REQUIRE(ctx, max_utts >= 1 && max_utts <= 65535, "dualpath: max_utts = %d out of range [1, 65535]", max_utts);
  CCX_REQUIRE(ctx, max_tokens >= 2 * dims->segment && max_tokens <= (1 << 24), "dualpath: max_tokens = %d out of range [2 segment, 2^24]", max_tokens);
  ccx_dualpath* s = new ccx_dualpath();
  s->ctx = ctx; s->store.ctx = ctx; s->d = *dims;
  s->max_tokens = max_tokens / dims->segment * dims->segment;
  s->max_utts = max_utts;
  *out = s;
  return CCX_OK;
}

void ccx_dualpath_destroy(ccx_dualpath* s) {
  if (!s) return;
  s->store.free_all();
  delete s;
}

int ccx_dualpath_set_tensor(ccx_dualpath* s, const char* name, const float* data, int64_t numel) {
  if (!s) return CCX_ERR_ARG;
  CCX_REQUIRE(s->ctx, !s->finalized && name && data && numel > 0, "dualpath: set_tensor bad arguments");
  const std::string nm(name);
  CCX_REQUIRE(s->ctx, nm.rfind("masknet.pos_enc.", 0) != 0,
              "dualpath: tensor '%s' belongs to use_global_pos_enc, which is not built (off in the published hparams)", name);
  CCX_REQUIRE(s->ctx, nm.find(".intra_linear.") == std::string::npos && nm.find(".inter_linear.") == std::string::npos,
              "dualpath: tensor '%s' belongs to linear_layer_after_inter_intra, which is not built (off in the published hparams)", name);
  CCX_REQUIRE(s->ctx, nm.rfind("encoder.", 0) == 0 || nm.rfind("decoder.", 0) == 0 || nm.rfind("masknet.", 0) == 0,
              "dualpath: unknown tensor name '%s'", name);
  const std::string pe_tail = ".pos_enc.pe";
  if (nm.size() > pe_tail.size() && nm.compare(nm.size() - pe_tail.size(), pe_tail.size(), pe_tail) == 0) return CCX_OK;   // a buffer: recomputed
  return s->store.stage(name, data, numel);
}

int ccx_dualpath_finalize(ccx_dualpath* s) {
  if (!s) return CCX_ERR_ARG;
  CCX_REQUIRE(s->ctx, !s->finalized, "dualpath: finalize called twice");
  const ccx_dualpath_dims& d = s->d;
  const int F = d.d_ffn, NS = d.n_spk;
  {
    CCX_NEED(s->store, we, "encoder.conv1d.weight", D, 1, d.kernel);
    CCX_NEED(s->store, wd, "decoder.weight", D, 1, d.kernel);
    CCX_NEED(s->store, ng, "masknet.norm.weight", D); CCX_NEED(s->store, nb, "masknet.norm.bias", D);
    CCX_NEED(s->store, wi, "masknet.conv1d.weight", D, D, 1);
    CCX_NEED(s->store, pr, "masknet.prelu.weight", 1);
    CCX_NEED(s->store, wf, "masknet.conv2d.weight", D * NS, D, 1, 1); CCX_NEED(s->store, bf, "masknet.conv2d.bias", D * NS);
    CCX_NEED(s->store, wo, "masknet.output.0.weight", D, D, 1); CCX_NEED(s->store, bo, "masknet.output.0.bias", D);
    CCX_NEED(s->store, wg, "masknet.output_gate.0.weight", D, D, 1); CCX_NEED(s->store, bg, "masknet.output_gate.0.bias", D);
    CCX_NEED(s->store, wend, "masknet.end_conv1x1.weight", D, D, 1);
    CCX_TRY(s->store.upload(&s->w_enc, we->data)); CCX_TRY(s->store.upload(&s->w_dec, wd->data));
    CCX_TRY(s->store.upload(&s->gn0_g, ng->data)); CCX_TRY(s->store.upload(&s->gn0_b, nb->data));
    CCX_TRY(s->store.upload_bf16(&s->W_in, wi->data));
    CCX_TRY(s->store.upload(&s->prelu, pr->data));
    CCX_TRY(s->store.upload_bf16(&s->W_fc, wf->data)); CCX_TRY(s->store.upload(&s->b_fc, bf->data));
    std::vector<float> wog(wo->data), bog(bo->data);                 // tanh branch rows 0 .. 255, gate branch rows 256 .. 511: one GEMM
    wog.insert(wog.end(), wg->data.begin(), wg->data.end());
    bog.insert(bog.end(), bg->data.begin(), bg->data.end());
    CCX_TRY(s->store.upload_bf16(&s->W_og, wog)); CCX_TRY(s->store.upload(&s->b_og, bog));
    CCX_TRY(s->store.upload_bf16(&s->W_end, wend->data));
  }
  s->intra.resize(d.n_blocks);
  s->inter.resize(d.n_blocks);
  for (int i = 0; i < d.n_blocks; i++) {
    const std::string b = "masknet.dual_mdl." + std::to_string(i);
    CCX_TRY(sb_load_stack(s->store, b + ".intra_mdl", b + ".intra_norm", d.n_layers, D, F, s->intra[i]));
    CCX_TRY(sb_load_stack(s->store, b + ".inter_mdl", b + ".inter_norm", d.n_layers, D, F, s->inter[i]));
  }
  s->store.staged.clear();
  // positional encoding table (interleaved sin / cos), long enough for a chunk and for the longest inter-chunk sequence
  const int max_chunks = s->max_tokens / d.segment;
  s->pe_len = d.segment > max_chunks ? d.segment : max_chunks;
  CCX_TRY(s->store.upload(&s->pe, sb_pos_enc_table(s->pe_len, D)));
  // frames of a call never exceed half its token rows (S K / 2 = L + gap + K / 2 per utterance)
  const size_t T = (size_t)s->max_tokens, Fr = T / 2 + 1, U = (size_t)s->max_utts;
  CCX_TRY(s->store.alloc(&s->feats, Fr * D, true)); CCX_TRY(s->store.alloc(&s->xf, Fr * D, true));
  CCX_TRY(s->store.alloc(&s->x, T * D, true)); CCX_TRY(s->store.alloc(&s->h, T * D, true)); CCX_TRY(s->store.alloc(&s->y, T * D, true));
  CCX_TRY(s->store.alloc(&s->xn, T * D, true)); CCX_TRY(s->store.alloc(&s->qkv, T * 3 * D, true)); CCX_TRY(s->store.alloc(&s->att, T * D, true));
  CCX_TRY(s->store.alloc(&s->hid, T * F, true)); CCX_TRY(s->store.alloc(&s->fc, T * NS * D, true));
  CCX_TRY(s->store.alloc(&s->ya, Fr * NS * D, true)); CCX_TRY(s->store.alloc(&s->g2, Fr * NS * 2 * D, true));
  CCX_TRY(s->store.alloc(&s->yb, Fr * NS * D, true)); CCX_TRY(s->store.alloc(&s->mk, Fr * NS * D, true));
  CCX_TRY(s->store.alloc(&s->part, 2 * U * CCX_DP_GN_PARTS, true));
  CCX_TRY(s->store.alloc(&s->utt, U, true));
  CCX_TRY(s->store.alloc(&s->seq_intra, 3 * (size_t)max_chunks, true)); CCX_TRY(s->store.alloc(&s->seq_inter, 3 * U * d.segment, true));
  CCX_TRY(s->store.alloc(&s->gn_tok, 2 * U, true)); CCX_TRY(s->store.alloc(&s->gn_frame, 2 * U, true));
  s->finalized = true;
  return CCX_OK;
}

int ccx_dualpath_separate(ccx_dualpath* s, const float* mix, int64_t stride, const int* n_samples, int B, float* out, void* stream_) {
  if (!s) return CCX_ERR_ARG;
  ccx_ctx* ctx = s->ctx;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, s->finalized && mix && n_samples && out && B >= 1 && B <= s->max_utts, "dualpath_separate: bad arguments (B=%d, max %d)", B, s->max_utts);
  const ccx_dualpath_dims& d = s->d;
  const int K = d.segment, P = K / 2, NS = d.n_spk;
  // ---- host-side ragged bookkeeping (tiny) ----
  std::vector<ccx_dp_utt> utt(B);
  long n_tok = 0, n_frame = 0;
  int max_S = 0, max_L = 0;
  for (int b = 0; b < B; b++) {
    CCX_REQUIRE(ctx, n_samples[b] >= d.kernel && n_samples[b] <= stride, "dualpath_separate: utterance %d has %d samples (need >= %d, <= stride)", b,
                n_samples[b], d.kernel);
    ccx_dp_utt& u = utt[b];
    memset(&u, 0, sizeof(u));
    u.T = n_samples[b];
    u.L = (n_samples[b] - d.kernel) / d.stride + 1;
    u.gap = K - (P + u.L % K) % K;
    u.S = 2 * (u.L + u.gap + P) / K;
    u.tok0 = (int)n_tok; u.frame0 = (int)n_frame;
    n_tok += (long)u.S * K; n_frame += u.L;
    CCX_REQUIRE(ctx, n_tok <= s->max_tokens, "dualpath_separate: the chunk rows of utterances 0 .. %d (%ld) exceed capacity %d", b, n_tok, s->max_tokens);
    max_S = std::max(max_S, u.S); max_L = std::max(max_L, u.L);
  }
  std::vector<int> sq_intra, sq_inter, gn_tok(2 * B), gn_frame(2 * B);
  for (int b = 0; b < B; b++) {
    const ccx_dp_utt& u = utt[b];
    for (int c = 0; c < u.S; c++) { sq_intra.push_back(u.tok0 + c * K); sq_intra.push_back(1); sq_intra.push_back(K); }
    for (int k = 0; k < K; k++) { sq_inter.push_back(u.tok0 + k); sq_inter.push_back(K); sq_inter.push_back(u.S); }
    gn_tok[2 * b] = u.tok0; gn_tok[2 * b + 1] = u.S * K;
    gn_frame[2 * b] = u.frame0; gn_frame[2 * b + 1] = u.L;
  }
  const int n_intra = (int)sq_intra.size() / 3, n_inter = (int)sq_inter.size() / 3;
#define UP(dst, vec) CCX_HIP(ctx, hipMemcpyAsync(dst, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, st))
  UP(s->utt, utt); UP(s->seq_intra, sq_intra); UP(s->seq_inter, sq_inter); UP(s->gn_tok, gn_tok); UP(s->gn_frame, gn_frame);
#undef UP
  CCX_HIP(ctx, hipStreamSynchronize(st));  // host staging vectors go out of scope

  const int nt = (int)n_tok, nf = (int)n_frame;
  CCX_TRY(ccx_launch_dp_encoder(ctx, mix, (long)stride, s->utt, B, max_L, d.kernel, s->w_enc, s->feats, st));
  CCX_TRY(ccx_launch_dp_group_norm(ctx, s->feats, s->gn_frame, B, max_L, s->gn0_g, s->gn0_b, nullptr, nullptr, s->xn, s->part, st));
  CCX_TRY(dp_gemm(ctx, EPI_F32, s->xn, s->W_in, nf, D, D, nullptr, s->xf, nullptr, st));
  CCX_TRY(ccx_launch_dp_segment(ctx, s->xf, s->utt, B, K, max_S, s->x, st));
  for (int i = 0; i < d.n_blocks; i++) {
    CCX_TRY(dp_run_transformer(s, s->intra[i], s->seq_intra, n_intra, K, 0, nt, B, max_S, st));
    CCX_TRY(dp_run_transformer(s, s->inter[i], s->seq_inter, n_inter, max_S, 1, nt, B, max_S, st));
  }
  CCX_TRY(ccx_launch_prelu_bf16(ctx, s->x, s->prelu, s->xn, (long)nt * D, "dp_prelu_kernel", st));
  CCX_TRY(dp_gemm(ctx, EPI_F32, s->xn, s->W_fc, nt, NS * D, D, s->b_fc, s->fc, nullptr, st));
  CCX_TRY(ccx_launch_dp_overlap_add(ctx, s->fc, s->utt, B, K, max_L, NS, s->ya, st));
  CCX_TRY(dp_gemm(ctx, EPI_F32, s->ya, s->W_og, nf * NS, 2 * D, D, s->b_og, s->g2, nullptr, st));
  CCX_TRY(ccx_launch_dp_gate(ctx, s->g2, s->yb, (long)nf * NS, st));
  CCX_TRY(dp_gemm(ctx, EPI_F32, s->yb, s->W_end, nf * NS, D, D, nullptr, s->mk, nullptr, st));
  return ccx_launch_dp_decoder(ctx, s->feats, s->mk, s->utt, B, d.kernel, NS, s->w_dec, out, (long)stride, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the kernels as stand-alone operators
// ---------------------------------------------------------------------------------------------------------------------------------
#define DP_BUF(field, need)                                                                                                          \
  do {                                                                                                                               \
    CCX_REQUIRE(ctx, d->field != nullptr, "ccx_dualpath_op: %s is NULL", #field);                                                    \
    CCX_REQUIRE(ctx, ccx_aligned16(d->field), "ccx_dualpath_op: %s is not 16-byte aligned", #field);                                 \
    CCX_REQUIRE(ctx, d->field##_elems >= (int64_t)(need), "ccx_dualpath_op: %s is accessed up to element %ld, %s_elems=%ld", #field, \
                (long)(need), #field, (long)d->field##_elems);                                                                       \
  } while (0)
#define DP_PARAM(field, count)                                                                                                       \
  do {                                                                                                                               \
    CCX_REQUIRE(ctx, d->field != nullptr, "ccx_dualpath_op: %s is NULL", #field);                                                    \
    CCX_REQUIRE(ctx, ccx_aligned16(d->field), "ccx_dualpath_op: %s is not 16-byte aligned", #field);                                 \
    CCX_REQUIRE(ctx, d->field##_elems == (int64_t)(count), "ccx_dualpath_op: %s holds %ld elements (%s_elems), the kernel reads %ld", \
                #field, (long)d->field##_elems, #field, (long)(count));                                                              \
  } while (0)
#define DP_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

int ccx_dualpath_op(ccx_ctx* ctx, int op, const ccx_dualpath_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dualpath_op: desc is NULL");
  CCX_REQUIRE(ctx, op >= CCX_DP_ATTENTION && op <= CCX_DP_PRELU, "ccx_dualpath_op: unknown op %d", op);
  const bool frame_op = op == CCX_DP_ENCODER || op == CCX_DP_DECODER;
  const bool chunk_op = op == CCX_DP_SEGMENT || op == CCX_DP_OVERLAP_ADD || op == CCX_DP_PE_ADD;
  const int rows = d->rows, frames = d->frames, K = d->segment, kernel = d->kernel;
  if (!frame_op) CCX_REQUIRE(ctx, rows >= 1 && rows <= (1 << 24), "ccx_dualpath_op: rows = %d out of range [1, 2^24]", rows);
  if (frame_op || op == CCX_DP_SEGMENT || op == CCX_DP_OVERLAP_ADD)
    CCX_REQUIRE(ctx, frames >= 1 && frames <= (1 << 24), "ccx_dualpath_op: frames = %d out of range [1, 2^24]", frames);
  if (op == CCX_DP_OVERLAP_ADD || op == CCX_DP_DECODER)
    CCX_REQUIRE(ctx, d->n_spk >= 1 && d->n_spk <= 3, "ccx_dualpath_op: n_spk = %d out of range [1, 3]", d->n_spk);
  if (op == CCX_DP_GROUP_NORM || op == CCX_DP_PE_ADD) CCX_REQUIRE(ctx, d->mode == 0 || d->mode == 1, "ccx_dualpath_op: mode = %d must be 0 or 1", d->mode);
  if (frame_op || chunk_op || op == CCX_DP_GROUP_NORM)
    CCX_REQUIRE(ctx, d->n_utt >= 1 && d->n_utt <= 65535, "ccx_dualpath_op: n_utt = %d out of range [1, 65535]", d->n_utt);
  CCX_REQUIRE(ctx, d->out != d->in && (op == CCX_DP_GROUP_NORM || d->out != d->in2), "ccx_dualpath_op: out aliases in or in2");
  const int NS = d->n_spk;
  int max_len = 0, max_S = 0, max_L = 0, max_rows = 0;
  std::vector<int> tab;
  std::vector<ccx_dp_utt> utt;
  if (op == CCX_DP_ATTENTION) {
    CCX_REQUIRE(ctx, d->n_seq >= 1 && d->n_seq <= (1 << 20), "ccx_dualpath_op: n_seq = %d out of range [1, 2^20]", d->n_seq);
    CCX_REQUIRE(ctx, d->seq_first && d->seq_stride && d->seq_len, "ccx_dualpath_op: seq_first, seq_stride or seq_len is NULL");
    for (int i = 0; i < d->n_seq; i++) {
      const int f = d->seq_first[i], sd = d->seq_stride[i], len = d->seq_len[i];
      CCX_REQUIRE(ctx, len >= 1, "ccx_dualpath_op: seq_len[%d] = %d, a sequence needs at least one token", i, len);
      CCX_REQUIRE(ctx, sd >= 1, "ccx_dualpath_op: seq_stride[%d] = %d must be positive", i, sd);
      CCX_REQUIRE(ctx, f >= 0 && (int64_t)f + (int64_t)(len - 1) * sd < rows, "ccx_dualpath_op: seq_first[%d] = %d, seq_stride[%d] = %d, seq_len[%d] = %d leave the %d rows",
                  i, f, i, sd, i, len, rows);
      tab.push_back(f); tab.push_back(sd); tab.push_back(len);
      max_len = std::max(max_len, len);
    }
    DP_BUF(in, (int64_t)rows * 3 * D);
    DP_BUF(out, (int64_t)rows * D);
  } else if (op == CCX_DP_GROUP_NORM) {
    CCX_REQUIRE(ctx, d->utt_row0 && d->utt_rows, "ccx_dualpath_op: utt_row0 or utt_rows is NULL");
    for (int u = 0; u < d->n_utt; u++) {
      const int r0 = d->utt_row0[u], n = d->utt_rows[u];
      CCX_REQUIRE(ctx, n >= 1, "ccx_dualpath_op: utt_rows[%d] = %d, an utterance needs at least one row", u, n);
      CCX_REQUIRE(ctx, r0 >= 0 && r0 <= rows && n <= rows - r0, "ccx_dualpath_op: utt_row0[%d] = %d, utt_rows[%d] = %d leave the %d rows", u, r0, u, n, rows);
      tab.push_back(r0); tab.push_back(n);
      max_rows = std::max(max_rows, n);
    }
    DP_BUF(in, (int64_t)rows * D);
    DP_BUF(out, (int64_t)rows * D);
    if (d->mode == 0) DP_BUF(in2, (int64_t)rows * D);
    DP_PARAM(w, D); DP_PARAM(w2, D);
  } else if (chunk_op) {
    CCX_REQUIRE(ctx, K >= 2 && K <= 256 && K % 2 == 0, "ccx_dualpath_op: segment = %d must be even and in [2, 256]", K);
    CCX_REQUIRE(ctx, d->utt_tok0 && d->utt_frame0 && d->utt_L && d->utt_gap && d->utt_S, "ccx_dualpath_op: utt_tok0, utt_frame0, utt_L, utt_gap or utt_S is NULL");
    for (int u = 0; u < d->n_utt; u++) {
      ccx_dp_utt v;
      memset(&v, 0, sizeof(v));
      v.tok0 = d->utt_tok0[u]; v.frame0 = d->utt_frame0[u]; v.L = d->utt_L[u]; v.gap = d->utt_gap[u]; v.S = d->utt_S[u];
      CCX_REQUIRE(ctx, v.L >= 1 && v.L <= (1 << 24), "ccx_dualpath_op: utt_L[%d] = %d out of range [1, 2^24]", u, v.L);
      const int gap = K - (K / 2 + v.L % K) % K;
      CCX_REQUIRE(ctx, v.gap == gap, "ccx_dualpath_op: utt_gap[%d] = %d, %d frames in chunks of %d leave a gap of %d", u, v.gap, v.L, K, gap);
      CCX_REQUIRE(ctx, v.S == 2 * (v.L + gap + K / 2) / K, "ccx_dualpath_op: utt_S[%d] = %d, %d frames in chunks of %d make %d chunks", u, v.S, v.L, K,
                  2 * (v.L + gap + K / 2) / K);
      CCX_REQUIRE(ctx, v.tok0 >= 0 && (int64_t)v.tok0 + (int64_t)v.S * K <= rows, "ccx_dualpath_op: utt_tok0[%d] = %d with %d chunks of %d leaves the %d rows", u,
                  v.tok0, v.S, K, rows);
      if (op != CCX_DP_PE_ADD)
        CCX_REQUIRE(ctx, v.frame0 >= 0 && (int64_t)v.frame0 + v.L <= frames, "ccx_dualpath_op: utt_frame0[%d] = %d with %d frames leaves the %d frames", u,
                    v.frame0, v.L, frames);
      utt.push_back(v);
      max_S = std::max(max_S, v.S); max_L = std::max(max_L, v.L);
    }
    if (op == CCX_DP_SEGMENT) { DP_BUF(in, (int64_t)frames * D); DP_BUF(out, (int64_t)rows * D); }
    if (op == CCX_DP_OVERLAP_ADD) { DP_BUF(in, (int64_t)rows * D * NS); DP_BUF(out, (int64_t)frames * NS * D); }
    if (op == CCX_DP_PE_ADD) {
      DP_BUF(in, (int64_t)rows * D); DP_BUF(out, (int64_t)rows * D);
      const int need = d->mode ? max_S : K;
      CCX_REQUIRE(ctx, d->w_elems % D == 0, "ccx_dualpath_op: w_elems = %ld is no multiple of 256", (long)d->w_elems);
      DP_BUF(w, (int64_t)need * D);
    }
  } else if (frame_op) {
    CCX_REQUIRE(ctx, kernel >= 2 && kernel <= 32 && kernel % 2 == 0, "ccx_dualpath_op: kernel = %d must be even and in [2, 32]", kernel);
    CCX_REQUIRE(ctx, d->utt_frame0 && d->utt_L && d->utt_T, "ccx_dualpath_op: utt_frame0, utt_L or utt_T is NULL");
    const int64_t sstride = op == CCX_DP_ENCODER ? d->in_stride : d->out_stride;
    CCX_REQUIRE(ctx, sstride >= kernel && sstride <= (1 << 30), "ccx_dualpath_op: %s = %ld out of range [kernel, 2^30]",
                op == CCX_DP_ENCODER ? "in_stride" : "out_stride", (long)sstride);
    for (int u = 0; u < d->n_utt; u++) {
      ccx_dp_utt v;
      memset(&v, 0, sizeof(v));
      v.frame0 = d->utt_frame0[u]; v.L = d->utt_L[u]; v.T = d->utt_T[u];
      CCX_REQUIRE(ctx, v.L >= 1, "ccx_dualpath_op: utt_L[%d] = %d, an utterance needs at least one frame", u, v.L);
      CCX_REQUIRE(ctx, v.T >= (op == CCX_DP_ENCODER ? kernel : 1) && v.T <= sstride, "ccx_dualpath_op: utt_T[%d] = %d out of range [%d, %ld]", u, v.T,
                  op == CCX_DP_ENCODER ? kernel : 1, (long)sstride);
      if (op == CCX_DP_ENCODER)
        CCX_REQUIRE(ctx, v.L == (v.T - kernel) / (kernel / 2) + 1, "ccx_dualpath_op: utt_L[%d] = %d, %d samples make %d frames", u, v.L, v.T,
                    (v.T - kernel) / (kernel / 2) + 1);
      CCX_REQUIRE(ctx, v.frame0 >= 0 && (int64_t)v.frame0 + v.L <= frames, "ccx_dualpath_op: utt_frame0[%d] = %d with %d frames leaves the %d frames", u,
                  v.frame0, v.L, frames);
      utt.push_back(v);
      max_L = std::max(max_L, v.L);
    }
    DP_PARAM(w, (int64_t)D * kernel);
    if (op == CCX_DP_ENCODER) { DP_BUF(in, (int64_t)d->n_utt * d->in_stride); DP_BUF(out, (int64_t)frames * D); }
    else { DP_BUF(in, (int64_t)frames * D); DP_BUF(in2, (int64_t)frames * NS * D); DP_BUF(out, (int64_t)d->n_utt * d->out_stride * NS); }
  } else if (op == CCX_DP_GATE) {
    DP_BUF(in, (int64_t)rows * 2 * D); DP_BUF(out, (int64_t)rows * D);
  } else {  // CCX_DP_PRELU
    DP_BUF(in, (int64_t)rows * D); DP_BUF(out, (int64_t)rows * D);
    DP_PARAM(w, 1);
  }

  ccx_op_scratch sc;
  int* d_tab = nullptr;
  ccx_dp_utt* d_utt = nullptr;
  float* d_part = nullptr;
  if (!tab.empty()) DP_HIP(sc.upload(&d_tab, (const int*)tab.data(), tab.size()));
  if (!utt.empty()) DP_HIP(sc.upload(&d_utt, (const ccx_dp_utt*)utt.data(), utt.size()));
  if (op == CCX_DP_GROUP_NORM) DP_HIP(sc.alloc(&d_part, (size_t)2 * d->n_utt * CCX_DP_GN_PARTS));
  int rc = CCX_OK;
  switch (op) {
    case CCX_DP_ATTENTION:
      rc = ccx_launch_dp_attention(ctx, (const bf16_t*)d->in, d_tab, d->n_seq, max_len, (bf16_t*)d->out, st);
      break;
    case CCX_DP_GROUP_NORM:
      rc = ccx_launch_dp_group_norm(ctx, (const float*)d->in, d_tab, d->n_utt, max_rows, (const float*)d->w, (const float*)d->w2,
                                    d->mode == 0 ? (const float*)d->in2 : nullptr, d->mode == 0 ? (float*)d->out : nullptr,
                                    d->mode == 1 ? (bf16_t*)d->out : nullptr, d_part, st);
      break;
    case CCX_DP_SEGMENT:
      rc = ccx_launch_dp_segment(ctx, (const float*)d->in, d_utt, d->n_utt, K, max_S, (float*)d->out, st);
      break;
    case CCX_DP_OVERLAP_ADD:
      rc = ccx_launch_dp_overlap_add(ctx, (const float*)d->in, d_utt, d->n_utt, K, max_L, NS, (bf16_t*)d->out, st);
      break;
    case CCX_DP_PE_ADD:
      rc = ccx_launch_dp_pe_add(ctx, (const float*)d->in, d_utt, d->n_utt, K, max_S, d->mode, (const float*)d->w, (float*)d->out, st);
      break;
    case CCX_DP_GATE:
      rc = ccx_launch_dp_gate(ctx, (const float*)d->in, (bf16_t*)d->out, rows, st);
      break;
    case CCX_DP_ENCODER:
      rc = ccx_launch_dp_encoder(ctx, (const float*)d->in, (long)d->in_stride, d_utt, d->n_utt, max_L, kernel, (const float*)d->w, (float*)d->out, st);
      break;
    case CCX_DP_DECODER:
      rc = ccx_launch_dp_decoder(ctx, (const float*)d->in, (const float*)d->in2, d_utt, d->n_utt, kernel, NS, (const float*)d->w, (float*)d->out,
                                 (long)d->out_stride, st);
      break;
    default:
      rc = ccx_launch_prelu_bf16(ctx, (const float*)d->in, (const float*)d->w, (bf16_t*)d->out, (long)rows * D, "dp_prelu_kernel", st);
  }
  DP_HIP(hipStreamSynchronize(st));      // the scratch is freed on return
  return rc;
}

}  // extern "C"

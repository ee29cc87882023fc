// sb_softmax.h -- the wave-level softmax over S^T score tiles that the three separator attention kernels share (sep_attention_kernel,
// sep_attn_block_kernel, dp_attention_kernel).  Device-only.
//
// Layout: S^T = K Q^T per 16-key tile, so a lane owns ONE query column (l15 = lane & 15) and four keys of it: s[t][r] is the score of
// key key0 + 16 t + 4 h4 + r (h4 = lane >> 4).  The four lanes l15, l15 + 16, + 32, + 48 hold one query's 16 keys of a tile.  The
// exponentiated registers are, unchanged, the A operand of O = P V (row = query, k = key), whose accumulator rows are the queries
// 4 h4 + r: per-query values (alpha, the normaliser) are fetched per output row with sb_row_value.
//
// The one rounding rule, which the fp64 references under tests/ and their measured bounds rest on:
//   * the scale (log2 e / sqrt(head_dim)) is folded into the one fma in front of exp2; the running maximum is kept scaled;
//   * the normaliser sums the UNROUNDED p, tile-major, register-minor, per lane; the four lanes of a query meet only after the last
//     block (lane_xor16, then lane_xor32);
//   * p is rounded to bf16 only as the MFMA operand (sb_pack_p); O / l is rounded at the caller's store.
// NT = key tiles per block; FULL = all NT tiles are live, otherwise the first nk (tiles past nk are neither read nor written: their
// p would be an exact zero, which leaves every sum as it is).  Keys >= len score -inf; they can only sit in the tile that crosses len.
#pragma once
#include <math.h>
#include "ccx_common.h"

typedef __attribute__((ext_vector_type(4))) short bf16x4v;

// masked maximum of a query's scores over the block, UNSCALED (-1e30 at the least); masks s in place
template <int NT, bool FULL>
__device__ __forceinline__ float sb_block_max(f32x4 (&s)[NT], int nk, int key0, int len, int h4) {
  float mx = -1e30f;
#pragma unroll
  for (int t = 0; t < NT; t++)
    if (FULL || t < nk) {
      if (key0 + t * 16 + 16 > len) {
#pragma unroll
        for (int r = 0; r < 4; r++) s[t][r] = key0 + t * 16 + 4 * h4 + r >= len ? -INFINITY : s[t][r];
      }
#pragma unroll
      for (int r = 0; r < 4; r++) mx = fmaxf(mx, s[t][r]);
    }
  mx = fmaxf(mx, lane_xor16(mx));
  return fmaxf(mx, lane_xor32(mx));
}

// s <- p = exp2(s scale - mx) of one tile (mx: the scaled maximum; exp2(-inf) = 0 for a masked key); ps += its four p in order
__device__ __forceinline__ void sb_exp_tile(f32x4& s, float scale_log2e, float mx, float& ps) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float pv = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -mx));
    s[r] = pv;
    ps += pv;
  }
}

// the same over a block of tiles; returns the lane's sum of p
template <int NT, bool FULL>
__device__ __forceinline__ float sb_block_exp(f32x4 (&s)[NT], int nk, float scale_log2e, float mx) {
  float ps = 0.f;
#pragma unroll
  for (int t = 0; t < NT; t++)
    if (FULL || t < nk) sb_exp_tile(s[t], scale_log2e, mx, ps);
  return ps;
}

// a tile of p as the bf16 A operand of O = P V: P[query l15][key 4 h4 + j]
__device__ __forceinline__ bf16x4v sb_pack_p(const f32x4& p) {
  union { bf16x4v v; uint32_t u[2]; } pa;
  pa.u[0] = pack_bf16x2(p[0], p[1]);
  pa.u[1] = pack_bf16x2(p[2], p[3]);
  return pa.v;
}

// v belongs to query l15 of the lane; the O tile holds queries 4 h4 + r on its rows: the value of row r
__device__ __forceinline__ float sb_row_value(float v, int h4, int r) { return __shfl(v, 4 * h4 + r, 64); }

// the normaliser of the lane's query after the last block: the four lanes that share a query meet
__device__ __forceinline__ float sb_query_sum(float l) {
  const float lt = l + lane_xor16(l);
  return lt + lane_xor32(lt);
}

// One online-softmax step over a block of score tiles: s <- p, (m_run, l_run) updated; returns alpha = exp2(m_old - m_new), by which
// the caller rescales its O rows (through sb_row_value) before it adds this block's P V.
template <int NT, bool FULL>
__device__ __forceinline__ float sb_online_step(f32x4 (&s)[NT], int nk, int key0, int len, int h4, float scale_log2e, float& m_run,
                                                float& l_run) {
  const float mx = fmaxf(m_run, sb_block_max<NT, FULL>(s, nk, key0, len, h4) * scale_log2e);
  const float alpha = __builtin_amdgcn_exp2f(m_run - mx);
  m_run = mx;
  l_run = l_run * alpha + sb_block_exp<NT, FULL>(s, nk, scale_log2e, mx);
  return alpha;
}

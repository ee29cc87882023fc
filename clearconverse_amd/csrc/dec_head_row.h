// dec_head_row.h -- the logit-filter core of a decode step's head: one logit row held in the registers of a 1024-thread block, as
// dec_select_kernel (decoder.hip) and dec_beam_topk_kernel (dec_beam.hip) both run it.  A kernel reads as its own prologue, then
//   head_load_row -> head_no_speech (first sampled step) -> head_filter<RULES>,
// then its own tail: the select kernel draws, truncates (dec_truncate.h) and steps the row's state machine; the beam kernel takes
// beam + 1 masked arg-max rounds out of the filtered registers.  A rule of the filter is changed here, once.
//
// Every function takes the caller's `tid` (= threadIdx.x): the ids are then the same expressions in the core and in the kernel's tail,
// which keeps the 1024-thread kernels at the parent's registers and scratch (profiles/dec_head_refactor_isa.txt).
// Thread t holds ids t * 4 + g * 4096 + j (g < kHeadV4, j < 4) in val[4 g + j]; bit 4 g + j of `sup` says that id is suppressed by the
// call's mask or lies behind the vocabulary.
//
// ORDER OF OPERATIONS.  Every sum and maximum is taken in one fixed order: the thread's 52 registers in index order, the wave by
// wave_reduce_sum / wave_reduce_max (DPP: (a + b) + (c + d)), the 16 wave results in wave order out of LDS.  That tree is NOT the xor
// butterfly of dec_trunc::block_sum_f, so the reductions of dec_truncate.h stay where they are.  Log-probabilities are formed as
// (x - mx_all) - lnorm, two numbers of the softmax's own magnitude, so a common offset of the logits does not cost them its ulp.
#pragma once
#include "decoder.h"

constexpr int kHeadV4 = 13;                          // float4 per thread
constexpr int kHeadMaxVocab = 1024 * kHeadV4 * 4;    // 53248 ids: what one block holds

// sh: 16 words of LDS; every thread returns the same value
__device__ __forceinline__ float block_reduce_max(float v, float* sh) {
  v = wave_reduce_max(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < nw; i++) r = fmaxf(r, sh[i]);
  return r;
}
__device__ __forceinline__ float block_reduce_sum(float v, float* sh) {
  v = wave_reduce_sum(v);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < nw; i++) r += sh[i];
  return r;
}

// block argmax of (v_, idx) over sh_v / sh_i (16 words each); ties -> lowest index, as torch.argmax on CPU
__device__ __forceinline__ void block_argmax(int tid, float v_, int idx, float& oval, int& oidx, float* sh_v, int* sh_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v_, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v_ || (ov == v_ && oi < idx)) { v_ = ov; idx = oi; }
  }
  __syncthreads();
  if ((tid & 63) == 0) { sh_v[tid >> 6] = v_; sh_i[tid >> 6] = idx; }
  __syncthreads();
  oval = sh_v[0]; oidx = sh_i[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); w++)
    if (sh_v[w] > oval || (sh_v[w] == oval && sh_i[w] < oidx)) { oval = sh_v[w]; oidx = sh_i[w]; }
}

// the id in register i of thread tid
__device__ __forceinline__ int head_id(int tid, int i) { return tid * 4 + (i >> 2) * 4096 + (i & 3); }

// ---- load the row + mask once (all loads issued before any use) ----
__device__ __forceinline__ unsigned long long head_load_row(int tid, const float* lg, const unsigned char* mask, int V, float (&val)[kHeadV4 * 4]) {
  unsigned long long sup = 0;  // bit i: element i of this thread is suppressed / out of range
#pragma unroll
  for (int i = 0; i < kHeadV4; i++) {
    const int v0 = tid * 4 + i * 4096;
    if (v0 + 3 < V) {
      const float4 f = *(const float4*)(lg + v0);
      const uchar4 m = *(const uchar4*)(mask + v0);
      val[4 * i] = f.x; val[4 * i + 1] = f.y; val[4 * i + 2] = f.z; val[4 * i + 3] = f.w;
      sup |= ((unsigned long long)((m.x ? 1 : 0) | (m.y ? 2 : 0) | (m.z ? 4 : 0) | (m.w ? 8 : 0))) << (4 * i);
    } else {  // n_vocab % 4 == 0 (checked on the host): a float4 is either fully inside or fully outside
      val[4 * i] = val[4 * i + 1] = val[4 * i + 2] = val[4 * i + 3] = -INFINITY;
      sup |= 0xFull << (4 * i);
    }
  }
  return sup;
}

// ---- no-speech probability from the raw logits at the SOT position (first sampling step) ----
// Formed on thread 0 only (0 elsewhere): the caller stores it from there.
__device__ __forceinline__ float head_no_speech(int tid, const float* lg, int no_speech, const float (&val)[kHeadV4 * 4], float* sh) {
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < kHeadV4 * 4; i++) mx = fmaxf(mx, val[i]);
  mx = block_reduce_max(mx, sh);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < kHeadV4 * 4; i++) sum += __builtin_amdgcn_exp2f((val[i] - mx) * 1.4426950408889634f);  // -inf -> 0
  sum = block_reduce_sum(sum, sh);
  return tid == 0 ? expf(lg[no_speech] - mx) / sum : 0.f;
}

// What the filter leaves beside the filtered row: the best allowed text id (bt, it) and timestamp (bs, is) -- value -inf and id
// 0x7fffffff where the set is empty --, mx_all = max(bt, bs), the log-normaliser relative to mx_all of the row as the step samples it,
// and whether the summed timestamp mass beats the best text token (then the step samples timestamps only; val keeps its text ids).
// RULES = false: one allowed set under (bt, it), no timestamp side.
struct HeadFilter {
  float bt, bs, mx_all, lnorm;
  int it, is;
  bool force_ts;
};

template <bool RULES>
__device__ __forceinline__ HeadFilter head_filter(int tid, const DecSelectParams& p, const DecSeqState& s, float (&val)[kHeadV4 * 4], unsigned long long sup,
                                                  float* sh, float* sh_v, int* sh_i) {
  HeadFilter f;
  const int V = p.n_vocab, i_gen = s.n_gen, tsb = p.timestamp_begin;
  if constexpr (RULES) {
    // ---- timestamp-rule state (ApplyTimestampRules) folded into two allowed id ranges ----
    // text ids   [t_lo, tsb):  empty on the first step (must start with a timestamp); only >= eot after
    //                          "text, timestamp" (a timestamp must be paired or followed by eot)
    // timestamps [s_lo, s_hi): >= the last timestamp (+1 unless it is still unpaired); empty after a
    //                          closed pair "timestamp, timestamp"; <= max_initial_timestamp on the first step
    // SuppressBlank only matters on the first step, where every text id is banned anyway.
    const bool last_ts = i_gen >= 1 && s.last_tok >= tsb;
    const bool pen_ts = i_gen < 2 || s.pen_tok >= tsb;
    int s_lo = tsb;
    if (s.last_ts_tok >= 0) s_lo = (last_ts && !pen_ts) ? s.last_ts_tok : s.last_ts_tok + 1;
    int s_hi = V;
    if (i_gen == 0 && p.max_initial_ts >= 0) s_hi = tsb + p.max_initial_ts + 1;
    if (last_ts && pen_ts) s_hi = s_lo;
    const int t_lo = (i_gen == 0) ? tsb : ((last_ts && !pen_ts) ? p.eot : 0);

    // pass 1 (registers): apply the filters in place (-inf) and take text / timestamp maxima
    float mx_text = -INFINITY, mx_ts = -INFINITY;
    int am_text = 0x7fffffff, am_ts = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) {
      const int v = head_id(tid, i);
      const bool is_text = v < tsb;
      const bool allowed = !((sup >> i) & 1) && (is_text ? (v >= t_lo) : (v >= s_lo && v < s_hi));
      const float x = allowed ? val[i] : -INFINITY;
      val[i] = x;
      const bool bt_ = is_text && x > mx_text, bs_ = !is_text && x > mx_ts;
      mx_text = bt_ ? x : mx_text; am_text = bt_ ? v : am_text;
      mx_ts = bs_ ? x : mx_ts; am_ts = bs_ ? v : am_ts;
    }
    block_argmax(tid, mx_text, am_text, f.bt, f.it, sh_v, sh_i);
    block_argmax(tid, mx_ts, am_ts, f.bs, f.is, sh_v, sh_i);
    f.mx_all = fmaxf(f.bt, f.bs);

    // pass 2 (registers): sum exp over text and over timestamps (relative to mx_all)
    float se_text = 0.f, se_ts = 0.f;
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) {
      const int v = head_id(tid, i);
      const float e = __builtin_amdgcn_exp2f((val[i] - f.mx_all) * 1.4426950408889634f);  // banned entries are -inf -> 0
      se_text += (v < tsb) ? e : 0.f;
      se_ts += (v < tsb) ? 0.f : e;
    }
    se_text = block_reduce_sum(se_text, sh);
    se_ts = block_reduce_sum(se_ts, sh);

    // timestamp_logprob > max_text_token_logprob  <=>  lse_ts > max_text (same normaliser)
    const float lse_ts = (se_ts > 0.f) ? f.mx_all + logf(se_ts) : -INFINITY;
    f.force_ts = lse_ts > f.bt;
    f.lnorm = logf(f.force_ts ? se_ts : se_text + se_ts);   // of the re-filtered logits
  } else {
    // ---- no ApplyTimestampRules (without_timestamps): one allowed set, one argmax, one softmax ----
    // allowed: not suppressed by the call's mask, and on the first sampled step, with SuppressBlank on, neither " " nor eot.
    // Timestamp ids and <|notimestamps|> are ids like any other here.
    const bool ban0 = p.suppress_blank && i_gen == 0;
    float mx = -INFINITY; int am = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) {
      const int v = head_id(tid, i);
      const bool allowed = !((sup >> i) & 1) && !(ban0 && (v == p.blank || v == p.eot));
      const float x = allowed ? val[i] : -INFINITY;
      val[i] = x;
      const bool b_ = x > mx;            // ids ascend with i: the lowest id of equal values stays
      mx = b_ ? x : mx; am = b_ ? v : am;
    }
    block_argmax(tid, mx, am, f.bt, f.it, sh_v, sh_i);
    f.bs = -INFINITY; f.is = 0x7fffffff; f.force_ts = false;
    f.mx_all = f.bt;
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) se += __builtin_amdgcn_exp2f((val[i] - f.mx_all) * 1.4426950408889634f);   // banned: -inf -> 0
    se = block_reduce_sum(se, sh);
    f.lnorm = logf(se);
  }
  return f;
}

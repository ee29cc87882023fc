// dec_truncate.h -- top_k / top_p / min_p truncation of one filtered logit row held in the registers of a 1024-thread block
// (the TRUNC instantiations of dec_select_kernel, decoder.hip; the rule: include/ccx.h ccx_decode_sampling_options).
//
// All three steps keep an upper set of the row in x, so the answer is ONE value: the smallest kept logit `cut`; the Gumbel loop of
// the select kernel then reads x < cut as -inf.  The two data-dependent bounds are found by a bitwise descent, most significant bit
// first, over the order-preserving 32-bit key of a float (key = bits | 0x80000000 for a clear sign bit, ~bits for a set one); a
// candidate key is turned back into the float it stands for and the row is compared against that, so -0 and +0 count as one value
// and a candidate that decodes to NaN holds nothing above it:
//   top_k : the largest key t with  count{x >= f(t)} >= k   -- the k-th largest value, multiplicity counted (32 counting passes)
//   top_p : the largest key t with  mass{x >= c1, x > f(t)} >= top_p * mass{x >= c1}; kept is x > f(t)       (32 mass passes)
//   min_p : x >= max + T * ln(min_p), the product and the sum rounded separately (no fma)
// mass(x) = exp2((x - m) * log2(e) / T) with m the row's maximum, so the largest term is exactly 1 and the total can neither vanish
// nor overflow at any temperature.
//
// DETERMINISM.  Every count and every mass is a reduction in one fixed order: the thread's 52 registers in index order, a 6-level xor
// butterfly inside the wave, the 16 wave totals in wave order out of LDS.  No atomics.  A term that is left out is added as +0, so
// the tree is the same for every candidate, and because fp32 rounding is monotone a mass over a larger set is never the smaller
// number: the descent's predicate is monotone in t and its result is the exact boundary of the predicate as computed.  One block
// owns one row, so nothing depends on the launch geometry.
#pragma once

namespace dec_trunc {

__device__ __forceinline__ float key_to_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// sh: 16 words of LDS; every thread returns the same total
__device__ __forceinline__ int block_sum_i(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  int r = 0;
  for (int i = 0; i < nw; i++) r += sh[i];
  return r;
}
__device__ __forceinline__ float block_sum_f(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < nw; i++) r += sh[i];
  return r;
}
__device__ __forceinline__ float block_min_f(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < nw; i++) r = fminf(r, sh[i]);
  return r;
}

// val: the thread's share of the row after EVERY filter (banned ids -inf, the text ids of a forced-timestamp row included);
// m: the row's maximum (> -inf: the caller skips a row with nothing allowed).  Returns the smallest kept logit; the maximum is always
// kept.  kept / kept_mass (thread 0 writes; null: not computed): |K| and the mass of K under softmax(x / T) over the whole row.
template <int N>
__device__ __forceinline__ float row_cut(const float (&val)[N], float m, float temperature, int top_k, float top_p, float min_p,
                                         float* sh_f, int* sh_i, int* kept, float* kept_mass) {
  const float scale = 1.4426950408889634f * (1.0f / temperature);
  // 1. top_k: c1 = the k-th largest value.  A row with fewer than k allowed ids ends below every finite key: nothing is cut.
  float c1 = -INFINITY;
  if (top_k > 0) {
    unsigned t = 0;
    for (int bit = 31; bit >= 0; bit--) {
      const unsigned cand = t | (1u << bit);
      const float tf = key_to_float(cand);
      int c = 0;
#pragma unroll
      for (int i = 0; i < N; i++) c += (val[i] >= tf) ? 1 : 0;
      c = block_sum_i(c, sh_i);
      if (c >= top_k) t = cand;
    }
    c1 = (t >= 0x00800000u) ? key_to_float(t) : -INFINITY;   // keys below 0x00800000 are -inf and the negative NaNs
  }
  // 2. top_p over the survivors of 1, renormalised: keep x iff the survivors strictly above it weigh less than top_p of them all
  float c2 = -INFINITY;        // exclusive: kept is x > c2
  if (top_p < 1.f) {
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const float e = __builtin_amdgcn_exp2f((val[i] - m) * scale);    // -inf -> 0
      s1 += (val[i] >= c1) ? e : 0.f;
    }
    s1 = block_sum_f(s1, sh_f);
    const float need = top_p * s1;
    unsigned t = 0;
    for (int bit = 31; bit >= 0; bit--) {
      const unsigned cand = t | (1u << bit);
      const float tf = key_to_float(cand);
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < N; i++) {
        const float e = __builtin_amdgcn_exp2f((val[i] - m) * scale);
        a += (val[i] >= c1 && val[i] > tf) ? e : 0.f;
      }
      a = block_sum_f(a, sh_f);
      if (a >= need) t = cand;
    }
    c2 = (t >= 0x00800000u) ? key_to_float(t) : -INFINITY;
  }
  // 3. min_p, in logit space: p_v >= min_p * p_max  <=>  x_v >= x_max + T * ln(min_p)
  const float c3 = (min_p > 0.f) ? __fadd_rn(m, __fmul_rn(temperature, logf(min_p))) : -INFINITY;
  // the cut as a value of the row: the smallest logit all three keep (the maximum passes every one of them)
  float lo = INFINITY;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const float x = val[i];
    const bool k = x > -INFINITY && x >= c1 && x > c2 && x >= c3;
    lo = k ? fminf(lo, x) : lo;
  }
  const float cut = fminf(block_min_f(lo, sh_f), m);
  if (kept || kept_mass) {
    int n = 0; float a = 0.f, s = 0.f;
#pragma unroll
    for (int i = 0; i < N; i++) {
      const float e = __builtin_amdgcn_exp2f((val[i] - m) * scale);
      n += (val[i] >= cut) ? 1 : 0;
      a += (val[i] >= cut) ? e : 0.f;
      s += e;
    }
    n = block_sum_i(n, sh_i);
    a = block_sum_f(a, sh_f);
    s = block_sum_f(s, sh_f);
    if (threadIdx.x == 0) {
      if (kept) *kept = n;
      if (kept_mass) *kept_mass = a / s;
    }
  }
  return cut;
}

}  // namespace dec_trunc

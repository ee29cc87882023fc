// decoder.hip -- Whisper TextDecoder single-token step kernels (K9/K10 in SURVEY.md section 2a).
//
// One decode step for B sequences is a fixed chain of small kernels that the host captures in a
// hipGraph (whisper.hip).  All per-sequence variation (current token, position, prompt vs
// sampling phase, timestamp-rule state, finished flag) lives in device arrays, so the captured
// graph is replayed unchanged for every step and no host round trip is needed inside the loop.
//
//  * dec_linear_kernel: "skinny" GEMM out[M<=64 rows, N] = act * W^T for the decoder's
//    weight-streaming linears.  W fragments go HBM -> VGPR directly (each weight byte is used
//    once per step, an LDS round trip would be pure overhead: cdna_hip_programming.md, "GEMV /
//    M <= 16 decode weights"); activations are LayerNorm-ed (or combined from split-KV attention
//    partials) into LDS once per block; v_mfma_f32_16x16x32_bf16 with the sequence index on the
//    MFMA column; the 4 waves of a block split K and reduce through LDS.
//  * dec_attention_kernel: single-query attention streaming K and V rows with 16-byte loads
//    (8 keys x 128 B per wave instruction), lane-group-local online softmax, split-KV partials
//    for the 1500-key cross attention.
//  * dec_select_kernel: SuppressBlank / SuppressTokens / ApplyTimestampRules + greedy argmax +
//    running sum-logprob + no-speech probability (openai-whisper decoding.py, restated in
//    oracle/whisper_ref.py) -- one block per sequence, device-side state machine.
#include <string>
#include "decoder.h"

// ------------------------------------------------------------------------------------------
// Embedding: x[b] = tok_emb[token[b]] + pos_emb[pos[b]]
// ------------------------------------------------------------------------------------------
__global__ void dec_embed_kernel(const float* __restrict__ tok_emb, const float* __restrict__ pos_emb,
                                 const int* __restrict__ cur_tok, const int* __restrict__ pos, float* __restrict__ x,
                                 int D) {
  const int b = blockIdx.x;
  const float4* te = (const float4*)(tok_emb + (long)cur_tok[b] * D);
  const float4* pe = (const float4*)(pos_emb + (long)pos[b] * D);
  float4* xo = (float4*)(x + (long)b * D);
  for (int i = threadIdx.x; i < D / 4; i += blockDim.x) {
    const float4 a = te[i], c = pe[i];
    xo[i] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
  }
}

#include "dec_ln.h"

// The shift DEPI_RESOLVE centres a row by before its bf16 copy (DecLinearParams::shift): the row's LayerNorm mean where it exceeds the
// row's std, else 0 -- a near-zero-mean row gains nothing from centring and keeps the uncentred arithmetic (and bits) it always had.
__device__ __forceinline__ float centre_shift(float mean, float rstd) { return fabsf(mean) * rstd > 1.f ? mean : 0.f; }

// Split-KV combine of one (row, head) = mh and 8-wide d chunk c, packed to bf16: out[d] = sum_s w_s o_s[d] / sum_s w_s l_s with
// w_s = 2^(m_s - max m).  All partial loads (nsplit <= 8) are issued up front; the slots past nsplit re-read slot 0 with weight 0.
// Shared by dec_combine_kernel and the ACT_COMBINE prologue of dec_linear_kernel.
__device__ __forceinline__ uint4 combine_partials(const float* part_o, const float* part_ml, int nsplit, int mh, int c) {
  const float2* ml = (const float2*)(part_ml + ((long)mh * nsplit) * 2);
  const float* ob = part_o + ((long)mh * nsplit) * 64 + 8 * c;
  float2 mlv[8];
  float4 oa[8], oc[8];
#pragma unroll
  for (int s = 0; s < 8; s++) {
    const int sc = s < nsplit ? s : 0;
    mlv[s] = ml[sc];
    oa[s] = *(const float4*)(ob + sc * 64);
    oc[s] = *(const float4*)(ob + sc * 64 + 4);
    if (s >= nsplit) mlv[s] = make_float2(-1e30f, 0.f);
  }
  float mx = -1e30f;
#pragma unroll
  for (int s = 0; s < 8; s++) mx = fmaxf(mx, mlv[s].x);
  float den = 0.f, o[8];
#pragma unroll
  for (int j = 0; j < 8; j++) o[j] = 0.f;
#pragma unroll
  for (int s = 0; s < 8; s++) {
    const float w = (s < nsplit) ? __builtin_amdgcn_exp2f(mlv[s].x - mx) : 0.f;
    den += w * mlv[s].y;
    o[0] += w * oa[s].x; o[1] += w * oa[s].y; o[2] += w * oa[s].z; o[3] += w * oa[s].w;
    o[4] += w * oc[s].x; o[5] += w * oc[s].y; o[6] += w * oc[s].z; o[7] += w * oc[s].w;
  }
  const float inv = 1.0f / den;
  uint4 pk;
  pk.x = pack_bf16x2(o[0] * inv, o[1] * inv); pk.y = pack_bf16x2(o[2] * inv, o[3] * inv);
  pk.z = pack_bf16x2(o[4] * inv, o[5] * inv); pk.w = pack_bf16x2(o[6] * inv, o[7] * inv);
  return pk;
}

// ------------------------------------------------------------------------------------------
// Skinny linear
// ------------------------------------------------------------------------------------------
// Every kernel of the decode chain is latency-bound (a 768x768 bf16 matrix is 4.6 KB per CU, and a
// slot of a dependent graph chain costs ~1.6 us even when empty -- tools/microbench_chain.hip), so
// the structure minimises instructions and dependent round trips on the one critical path:
//  1. each wave issues ALL weight loads of its K slice first (<= KMAX x NT 16-byte non-temporal
//     loads per lane: each weight byte is read once per step);
//  2. the activation prologue runs under that flight: LayerNorm of the residual rows (live rows
//     only, two at a time), or the split-KV attention combine, or nothing (bf16 activations are
//     loaded as fragments, also all up front);
//  3. MFMAs run out of registers; the 4 waves (K split) reduce through LDS.
// Residual adds are DEFERRED: out-proj / cross-out / FFN2 write split-K partial sums (DEPI_PARTIAL,
// grid.z = K split, so 4.7 MB matrices spread over 192 blocks instead of 48) and the NEXT
// LayerNorm prologue folds them in (x_eff = x_in + sum partials), block (0,*,0) writing x_eff to
// the other residual buffer (ping-pong: no block may see a half-updated stream).
// NW = 4 waves per block split K (kept as a template argument: kernel symbols and profile labels carry it).
// The depth-10 LayerNorm form (K = 1280) asks for two waves per SIMD: left alone the compiler hoists its prologue loads into 254 + 12
// registers (one block per CU, where the depth-8 form has two); held to 256 it takes 206 .. 209, no scratch.
template <int MT, int NT, int KMAX, int ACT, int EPI, int NW = 4>
__global__ __launch_bounds__(64 * NW, (KMAX > 8 && ACT == ACT_LN) ? 2 : 1) void dec_linear_kernel(DecLinearParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MROWS = 16 * MT;
  constexpr int BN = 16 * NT;
  constexpr int NTHR = 64 * NW;
  constexpr bool BF16IN = (ACT == ACT_BF16);
  constexpr int LNS = KMAX > 8 ? 5 : 4;  // float4 slots per lane of the LayerNorm prologue (32 KMAX columns per wave x 4 waves / 256)
  constexpr int LNR = KMAX > 8 ? 1 : 2;  // ... and rows a wave normalises per pass
  static_assert(NW == 4, "the LayerNorm / combine prologues and the launcher are written for four waves");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * BN;
  const int m0 = blockIdx.y * MROWS;
  const int K = p.K;
  const int lds_ld = K + 8;  // bf16 elements per LDS activation row (ACT_LN / ACT_COMBINE only)
  bf16_t* act_s = (bf16_t*)smem;
  float* red = (float*)(smem + (BF16IN ? 0 : ccx_align((size_t)MROWS * lds_ld * 2, 16)));

  const int l15 = lane & 15, h4 = lane >> 4;
  // K range of this block (grid.z split), then of this wave
  const int ksteps = K >> 5;
  const int per_z = (ksteps + gridDim.z - 1) / gridDim.z;
  const int kz0 = blockIdx.z * per_z;
  const int kz1 = (kz0 + per_z < ksteps) ? kz0 + per_z : ksteps;
  const int per_w = (kz1 - kz0 + NW - 1) / NW;
  const int ks0 = kz0 + wave * per_w;
  int nks = kz1 - ks0;
  nks = nks < 0 ? 0 : (nks > per_w ? per_w : nks);

  // Epilogue ownership: a thread finishes QUADS of 4 consecutive output columns of one row.  Quad qd = ((i * MT + j) * 64 + ln)
  // is exactly the f32x4 that lane ln of every wave holds for tile (i, j): row 16 j + (ln & 15), columns 16 i + 4 (ln >> 4) .. + 3.
  // The four waves' partial sums of a quad are therefore four ds_read_b128 at consecutive-lane addresses (conflict-free; the
  // former one-column-per-thread walk read single floats 64 apart: 4-way bank conflicts, 60 % of the kernel's LDS cycles).
  constexpr int QUADS = NT * MT * 64;
  constexpr int EPI_ITERS = (QUADS + NTHR - 1) / NTHR;
  // bias of this thread's columns and, for DEPI_SELF_QKV, the cache position of its rows: loaded up front so that the epilogue
  // has no dependent memory round trip of its own
  float4 bias_v[EPI_ITERS];
  float4 xold_v[EPI_ITERS];    // DEPI_RESOLVE: the residual tile this thread finishes
  float shift_v[EPI_ITERS];    // DEPI_RESOLVE: what its bf16 copy and statistics are centred by
  int pos_v[EPI_ITERS];
#pragma unroll
  for (int it = 0; it < EPI_ITERS; it++) {
    const int qd = tid + NTHR * it;
    const int ln = qd & 63, tj = (qd >> 6) % MT, ti = (qd >> 6) / MT;
    const int n_ = n0 + 16 * ti + 4 * (ln >> 4);
    bias_v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias && blockIdx.z == 0 && qd < QUADS) {
      if (n_ + 3 < p.N) bias_v[it] = *(const float4*)(p.bias + n_);
      else {
        if (n_ < p.N) bias_v[it].x = p.bias[n_];
        if (n_ + 1 < p.N) bias_v[it].y = p.bias[n_ + 1];
        if (n_ + 2 < p.N) bias_v[it].z = p.bias[n_ + 2];
      }
    }
    pos_v[it] = 0;
    if (EPI == DEPI_SELF_QKV) {
      const int m_ = m0 + 16 * tj + (ln & 15);
      pos_v[it] = p.pos[m_ < p.M ? m_ : p.M - 1];
    }
    xold_v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    shift_v[it] = 0.f;
    if (EPI == DEPI_RESOLVE && qd < QUADS) {
      const int m_ = m0 + 16 * tj + (ln & 15);
      xold_v[it] = *(const float4*)(p.xres + (long)(m_ < p.M ? m_ : p.M - 1) * p.N + (n_ + 3 < p.N ? n_ : 0));
      const float sh = p.shift ? p.shift[m_ < p.M ? m_ : p.M - 1] : 0.f;
      shift_v[it] = sh != 0.f ? sh + p.shift_c : 0.f;
    }
  }

  // ---------------- 1. weight (and bf16 activation) prefetch ----------------
  // W is stored fragment-packed (whisper.hip pack_mfma_rows): tile (n/16, k/32) holds the 64 lanes'
  // 16-byte A fragments back to back, so one wave load is 1 KB contiguous and successive k-steps
  // are successive KBs.  Rows >= N are zero padding inside the packed image.
  bf16x8 wf[NT][KMAX];
#pragma unroll
  for (int i = 0; i < NT; i++) {
    const long tile = (long)(blockIdx.x * NT + i) * ksteps + ks0;
    const bf16_t* wr = p.W + (tile * 64 + lane) * 8;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      const int kk = k < nks ? k : 0;  // clamp instead of branching: keeps the loads back to back
      wf[i][k] = __builtin_nontemporal_load((const bf16x8*)(wr + 512 * kk));
    }
  }
  bf16x8 af[MT][KMAX];
  if (BF16IN) {
    // row-major rows: 16 rows x 64 B per wave load, k-steps 64 B apart; act_packed (decoder.h): the rows' fragment image, 1 KB
    // contiguous per wave load like the weights, k-steps 1 KB apart.  Either way lane l gets row l & 15, columns 8 (l >> 4) .. + 7.
    const int kstride = p.act_packed ? 512 : 32;
#pragma unroll
    for (int j = 0; j < MT; j++) {
      int m = m0 + 16 * j + l15;
      m = m < p.M ? m : p.M - 1;  // rows >= M compute garbage that is never stored
      int mt = blockIdx.y * MT + j;
      mt = mt <= ((p.M - 1) >> 4) ? mt : ((p.M - 1) >> 4);   // (tiles behind the image: re-read its last one)
      const bf16_t* ar = p.act_packed ? p.act + (((long)mt * ksteps + (nks > 0 ? ks0 : 0)) * 64 + lane) * 8 : p.act + (long)m * p.lda + 8 * h4 + 32 * ks0;
#pragma unroll
      for (int k = 0; k < KMAX; k++) {
        const int kk = k < nks ? k : 0;
        af[j][k] = *(const bf16x8*)(ar + kstride * kk);
      }
    }
  }

  // ---------------- 2. activation staging ----------------
  if (ACT == ACT_LN) {
    // x_eff = x + sum of pending split-K partials; LayerNorm(x_eff) -> bf16 LDS rows.  A lane keeps LNS float4 of a row:
    // 4 (K <= 1024) with the prefetch depths 6 and 8, 5 (K <= 1280) with depth 10 -- K is one block's here, so KMAX bounds it.
    // A wave owns live rows wave, wave+4, ... and handles LNR of them per pass: two, or one in the 5-slot form, whose registers
    // two rows in flight would not fit beside the depth-10 weight prefetch without scratch or a lower occupancy.
    const int nv = K >> 2;
    int live = p.M - m0;
    live = live > MROWS ? MROWS : live;
    const bool writer = (blockIdx.x == 0 && blockIdx.z == 0 && p.x_out != nullptr);
    float4 g[LNS], bb[LNS];
#pragma unroll
    for (int i = 0; i < LNS; i++) {
      const int idx = lane + 64 * i;
      const int ic = idx < nv ? idx : 0;
      g[i] = ((const float4*)p.ln_g)[ic];
      bb[i] = ((const float4*)p.ln_b)[ic];
    }
    for (int r0 = wave; r0 < live; r0 += 4 * LNR) {
      float4 v[LNR][LNS];
      bool ok[LNR];
#pragma unroll
      for (int u = 0; u < LNR; u++) {
        const int r = r0 + 4 * u;
        ok[u] = r < live;
        const long row = (long)(m0 + (ok[u] ? r : r0)) * K;
        const float4* xr = (const float4*)(p.x + row);
#pragma unroll
        for (int i = 0; i < LNS; i++) {
          const int idx = lane + 64 * i;
          const int ic = idx < nv ? idx : 0;
          float4 a = xr[ic];
          float4 q[4];
#pragma unroll
          for (int s = 0; s < 4; s++)  // all slab loads issued together (clamped index, masked add)
            q[s] = ((const float4*)(p.pend + (long)(s < p.pend_n ? s : 0) * p.pend_stride + row))[ic];
#pragma unroll
          for (int s = 0; s < 4; s++) a = ln_add_pend(a, s < p.pend_n ? 1.f : 0.f, q[s]);
          if (idx >= nv) a = make_float4(0.f, 0.f, 0.f, 0.f);
          v[u][i] = a;
        }
      }
      float mean[LNR], rstd[LNR];
#pragma unroll
      for (int u = 0; u < LNR; u++) {
        float sm = 0.f;
#pragma unroll
        for (int i = 0; i < LNS; i++) sm += ln_sum4(v[u][i]);
        mean[u] = wave_reduce_sum(sm) / (float)K;
      }
#pragma unroll
      for (int u = 0; u < LNR; u++) {
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < LNS; i++) {
          const float t = ln_sq4(v[u][i], mean[u]);
          sq += (lane + 64 * i < nv) ? t : 0.f;
        }
        rstd[u] = rsqrtf(wave_reduce_sum(sq) / (float)K + p.eps);
      }
#pragma unroll
      for (int u = 0; u < LNR; u++) {
        if (!ok[u]) continue;
        const int r = r0 + 4 * u;
#pragma unroll
        for (int i = 0; i < LNS; i++) {
          const int idx = lane + 64 * i;
          if (idx < nv) {
            *(uint2*)(act_s + (long)r * lds_ld + 4 * idx) = ln_pack4(v[u][i], mean[u], rstd[u], g[i], bb[i]);
            if (writer) ((float4*)(p.x_out + (long)(m0 + r) * K))[idx] = v[u][i];
          }
        }
        if (p.ln_mean_out && blockIdx.x == 0 && blockIdx.z == 0 && lane == 0) p.ln_mean_out[m0 + r] = centre_shift(mean[u], rstd[u]);
      }
    }
    // dead rows of the 16-row MFMA tile: zeros
    for (int r = live + wave; r < MROWS; r += 4)
      for (int idx = lane; idx < (K >> 2); idx += 64) *(uint2*)(act_s + (long)r * lds_ld + 4 * idx) = make_uint2(0, 0);
    __syncthreads();
  } else if (ACT == ACT_COMBINE) {
    // combine split-KV attention partials: act[m][h*64+d] = sum_s w_s o_s[d] / sum_s w_s l_s.
    // One thread per (row, head, 8-wide d chunk); all partial loads (nsplit <= 8) issued up front.
    const int H = K >> 6;
    for (int e = tid; e < MROWS * H * 8; e += 256) {
      const int c = e & 7, h = (e >> 3) % H, r = e / (8 * H);
      const int m = m0 + r;
      const uint4 pk = m < p.M ? combine_partials(p.part_o, p.part_ml, p.nsplit, m * H + h, c) : make_uint4(0, 0, 0, 0);
      *(uint4*)(act_s + (long)r * lds_ld + h * 64 + 8 * c) = pk;
    }
    __syncthreads();
  }

  // ---------------- 3. MFMAs out of the prefetched registers ----------------
  f32x4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; i++)
#pragma unroll
    for (int j = 0; j < MT; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    if (k < nks) {
      if (!BF16IN) {
#pragma unroll
        for (int j = 0; j < MT; j++)
          af[j][k] = *(const bf16x8*)(act_s + (long)(16 * j + l15) * lds_ld + 8 * h4 + 32 * (ks0 + k));
      }
#pragma unroll
      for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < MT; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i][k], af[j][k], acc[i][j], 0, 0, 0);
    }
  }

  // ---------------- 4. cross-wave reduction through LDS + epilogue ----------------
  __syncthreads();  // everyone is done reading the activation image
#pragma unroll
  for (int i = 0; i < NT; i++)
#pragma unroll
    for (int j = 0; j < MT; j++) *(f32x4*)(red + (((wave * NT + i) * MT + j) * 64 + lane) * 4) = acc[i][j];
  __syncthreads();

#pragma unroll
  for (int it = 0; it < EPI_ITERS; it++) {
    const int qd = tid + NTHR * it;
    if (qd >= QUADS) break;
    const int ln = qd & 63, j = (qd >> 6) % MT, i = (qd >> 6) / MT;
    const int m = m0 + 16 * j + (ln & 15), n = n0 + 16 * i + 4 * (ln >> 4);
    if (EPI == DEPI_RESOLVE) {
      // whole waves stay together here (the statistics go through lane swaps); N is a multiple of the block's columns
      f32x4 v = *(const f32x4*)(red + (((0 * NT + i) * MT + j) * 64 + ln) * 4);
#pragma unroll
      for (int w = 1; w < NW; w++) v += *(const f32x4*)(red + (((w * NT + i) * MT + j) * 64 + ln) * 4);
      v[0] = (v[0] + bias_v[it].x) + xold_v[it].x; v[1] = (v[1] + bias_v[it].y) + xold_v[it].y;
      v[2] = (v[2] + bias_v[it].z) + xold_v[it].z; v[3] = (v[3] + bias_v[it].w) + xold_v[it].w;
      // the residual stays as it is; its bf16 copy and statistics are of the row centred by the shift (DecLinearParams)
      const float c0 = v[0] - shift_v[it], c1 = v[1] - shift_v[it], c2 = v[2] - shift_v[it], c3 = v[3] - shift_v[it];
      float s1 = (c0 + c1) + (c2 + c3);
      float s2 = fmaf(c3, c3, fmaf(c2, c2, fmaf(c1, c1, c0 * c0)));
      s1 += lane_xor16(s1); s2 += lane_xor16(s2);        // the four quads of a row's 16-column tile sit 16 lanes apart
      s1 += lane_xor32(s1); s2 += lane_xor32(s2);
      if (m < p.M && n < p.N) {
        *(float4*)(p.xres + (long)m * p.N + n) = make_float4(v[0], v[1], v[2], v[3]);
        uint2 pk;
        pk.x = pack_bf16x2(c0, c1); pk.y = pack_bf16x2(c2, c3);
        // out_packed: the quad's 8 bytes go into the fragment image the query kernel loads (N % 32 == 0)
        *(uint2*)(p.xb + (p.out_packed ? dec_frag_off(m, n, p.N >> 5) : (long)m * p.N + n)) = pk;
        if ((ln >> 4) == 0) p.st_out[(long)m * (p.N >> 4) + (n >> 4)] = make_float2(s1, s2);
      }
      continue;
    }
    if (n >= p.N || m >= p.M) continue;
    f32x4 v = *(const f32x4*)(red + (((0 * NT + i) * MT + j) * 64 + ln) * 4);
#pragma unroll
    for (int w = 1; w < NW; w++) v += *(const f32x4*)(red + (((w * NT + i) * MT + j) * 64 + ln) * 4);      // same order as before: w = 0..3
    v[0] += bias_v[it].x; v[1] += bias_v[it].y; v[2] += bias_v[it].z; v[3] += bias_v[it].w;
    const bool full = n + 3 < p.N;       // N is a multiple of 4 everywhere but a guard costs nothing
    if (EPI == DEPI_BF16_GELU) {
      // out_packed: the quad's 8 bytes go into the fragment image the next linear loads (N % 32 == 0, so every quad is full)
      bf16_t* o = (bf16_t*)p.out + (BF16IN && p.out_packed ? dec_frag_off(m, n, p.N >> 5) : (long)m * p.ldo + n);
      if (full) {
        uint2 pk;
        pk.x = pack_bf16x2(gelu_erf(v[0]), gelu_erf(v[1]));
        pk.y = pack_bf16x2(gelu_erf(v[2]), gelu_erf(v[3]));
        *(uint2*)o = pk;
      } else {
        for (int c = 0; c < 4 && n + c < p.N; c++) o[c] = f32_to_bf16(gelu_erf(v[c]));
      }
    } else if (EPI == DEPI_PARTIAL || EPI == DEPI_F32) {
      float* o = (float*)p.out + (EPI == DEPI_PARTIAL ? (long)blockIdx.z * p.pend_stride : 0L) + (long)m * p.ldo + n;
      if (full) *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      else
        for (int c = 0; c < 4 && n + c < p.N; c++) o[c] = v[c];
    } else if (EPI == DEPI_SELF_QKV) {
      const int D = p.K;  // d_model (a multiple of 64: a quad never straddles q / k / v or two heads)
      if (n < D) {
        *(float4*)((float*)p.out + (long)m * D + n) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        const int which = (n >= 2 * D);
        const int nn = n - (which ? 2 * D : D);
        const int hh = nn >> 6, d = nn & 63;
        const int H = D >> 6;
        bf16_t* cache = which ? p.cache_v : p.cache_k;
        const int sq = p.row_seq ? p.row_seq[m] : m;
        uint2 pk;
        pk.x = pack_bf16x2(v[0], v[1]);
        pk.y = pack_bf16x2(v[2], v[3]);
        *(uint2*)(cache + (((long)sq * H + hh) * p.cache_T + pos_v[it]) * 64 + d) = pk;
      }
    }
  }
}

// Stand-alone residual resolve + LayerNorm -> bf16 (input of the logits GEMV): one wave per row.
// NS = float4 slots per lane: 4 for K <= 1024, 5 for K <= 1280 (unrolled over the compile-time NS: the 4-slot form is unchanged).
template <int NS>
__global__ __launch_bounds__(256) void dec_resolve_ln_kernel(const float* __restrict__ x, const float* __restrict__ pend,
                                                             int pend_n, long pend_stride, const float* __restrict__ g,
                                                             const float* __restrict__ b, bf16_t* __restrict__ out,
                                                             float* __restrict__ x_out, int M, int K, float eps,
                                                             float* __restrict__ mean_out, int out_packed) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int nv = K >> 2;
  float4 v[NS], gg[NS], bb[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) {   // affine parameters first: no dependent load after the reductions
    const int idx = lane + 64 * i;
    const int ic = idx < nv ? idx : 0;
    gg[i] = ((const float4*)g)[ic];
    bb[i] = ((const float4*)b)[ic];
  }
  float sm = 0.f;
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const int idx = lane + 64 * i;
    const int ic = idx < nv ? idx : 0;
    float4 a = ((const float4*)(x + (long)m * K))[ic];
    float4 q[4];
#pragma unroll
    for (int s = 0; s < 4; s++) q[s] = ((const float4*)(pend + (long)(s < pend_n ? s : 0) * pend_stride + (long)m * K))[ic];
#pragma unroll
    for (int s = 0; s < 4; s++) a = ln_add_pend(a, s < pend_n ? 1.f : 0.f, q[s]);
    if (idx >= nv) a = make_float4(0.f, 0.f, 0.f, 0.f);
    v[i] = a;
    if (x_out && idx < nv) ((float4*)(x_out + (long)m * K))[idx] = a;   // resolved residual stream (ping-pong buffer)
    sm += ln_sum4(a);
  }
  const float mean = wave_reduce_sum(sm) / (float)K;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const float t = ln_sq4(v[i], mean);
    sq += (lane + 64 * i < nv) ? t : 0.f;
  }
  const float rstd = rsqrtf(wave_reduce_sum(sq) / (float)K + eps);
  if (mean_out && lane == 0) mean_out[m] = centre_shift(mean, rstd);
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const int idx = lane + 64 * i;
    // out_packed: the row's 8-byte pieces go into the fragment image the next linear loads (decoder.h dec_frag_off)
    if (idx < nv) *(uint2*)(out + (out_packed ? dec_frag_off(m, 4 * idx, K >> 5) : (long)m * K + 4 * idx)) = ln_pack4(v[i], mean, rstd, gg[i], bb[i]);
  }
}

// Stand-alone split-KV combine -> bf16 attention output [M][H*64] (used instead of the in-GEMV prologue for more than 16 rows:
// every weight-panel block would otherwise redo the whole combine).  Decode steps stream the whole key range per block instead
// (dec_cross_stream_kernel); ccx_whisper_decoder_logits keeps the split-KV kernels.
__global__ __launch_bounds__(256) void dec_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                          int nsplit, bf16_t* __restrict__ out, int M, int H) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // (row, head, 8-wide d chunk)
  if (e >= M * H * 8) return;
  const int c = e & 7, h = (e >> 3) % H, m = e / (8 * H);
  *(uint4*)(out + ((long)m * H + h) * 64 + 8 * c) = combine_partials(part_o, part_ml, nsplit, m * H + h, c);
}

__global__ void dec_gather_rows_kernel(const bf16_t* __restrict__ src, const int* __restrict__ idx, bf16_t* __restrict__ dst, int D) {
  if (idx[blockIdx.x] < 0) return;                 // row not taken in this pass (chunked prefill): dst keeps what it has
  const uint4* s4 = (const uint4*)(src + (long)idx[blockIdx.x] * D);
  uint4* d4 = (uint4*)(dst + (long)blockIdx.x * D);
  for (int i = threadIdx.x; i < D / 8; i += blockDim.x) d4[i] = s4[i];
}

int ccx_launch_dec_gather_rows(ccx_ctx* ctx, const bf16_t* src, const int* idx, bf16_t* dst, int n, int D, hipStream_t stream) {
  CCX_REQUIRE(ctx, src && idx && dst && n >= 1 && D % 8 == 0, "dec_gather_rows: bad arguments");
  hipLaunchKernelGGL(dec_gather_rows_kernel, dim3(n), dim3(128), 0, stream, src, idx, dst, D);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dec_combine(ccx_ctx* ctx, const float* part_o, const float* part_ml, int nsplit, bf16_t* out, int M, int H,
                           hipStream_t stream) {
  CCX_REQUIRE(ctx, nsplit >= 1 && nsplit <= 8, "dec_combine: nsplit out of range");
  ccx_prof_scope ps(ctx, stream, "dec_combine_kernel", 0.0, (double)M * H * nsplit * 66.0 * 4 + (double)M * H * 64 * 2);
  hipLaunchKernelGGL(dec_combine_kernel, dim3(ccx_cdiv(M * H * 8, 256)), dim3(256), 0, stream, part_o, part_ml, nsplit, out, M, H);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dec_resolve_ln(ccx_ctx* ctx, const float* x, const float* pend, int pend_n, long pend_stride, const float* g,
                              const float* b, bf16_t* out, float* x_out, int M, int K, float eps, hipStream_t stream,
                              float* mean_out, int out_packed) {
  CCX_REQUIRE(ctx, K % 4 == 0 && K <= 1280, "dec_resolve_ln: K=%d unsupported (a multiple of 4, at most 1280)", K);
  CCX_REQUIRE(ctx, !out_packed || K % 32 == 0, "dec_resolve_ln: the fragment image needs K=%d to be a multiple of 32", K);
  CCX_REQUIRE(ctx, x_out != x, "dec_resolve_ln: x_out must not alias x");
  // bytes: the residual rows and their pending slabs in, the bf16 rows (and the resolved fp32 rows) out
  ccx_prof_scope ps(ctx, stream, "dec_resolve_ln_kernel", 0.0, (double)M * K * (4.0 * (1 + pend_n) + 2.0 + (x_out ? 4.0 : 0.0)));
  if (K <= 1024)
    hipLaunchKernelGGL(dec_resolve_ln_kernel<4>, dim3(ccx_cdiv(M, 4)), dim3(256), 0, stream, x, pend, pend_n, pend_stride, g, b,
                       out, x_out, M, K, eps, mean_out, out_packed);
  else
    hipLaunchKernelGGL(dec_resolve_ln_kernel<5>, dim3(ccx_cdiv(M, 4)), dim3(256), 0, stream, x, pend, pend_n, pend_stride, g, b,
                       out, x_out, M, K, eps, mean_out, out_packed);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

template <int MT, int NT, int KMAX, int ACT, int EPI>
static int launch_dec_linear_inst(ccx_ctx* ctx, const DecLinearParams& p, int ksplit, hipStream_t stream) {
  const int MROWS = 16 * MT, BN = 16 * NT;
  size_t act_bytes = ACT == ACT_BF16 ? 0 : ccx_align((size_t)MROWS * (p.K + 8) * 2, 16);
  size_t red_bytes = (size_t)4 * NT * MT * 64 * 4 * 4;
  size_t lds = act_bytes + red_bytes;
  CCX_REQUIRE(ctx, lds <= 160 * 1024, "dec_linear: LDS %zu too large", lds);
  CCX_REQUIRE(ctx, ccx_cdiv(ccx_cdiv(p.K / 32, ksplit), 4) <= KMAX, "dec_linear: K=%d / split %d exceeds the prefetch depth %d", p.K, ksplit, KMAX);
  if (EPI == DEPI_RESOLVE) CCX_REQUIRE(ctx, p.xres && p.xb && p.st_out && ksplit == 1 && p.N % BN == 0, "dec_linear: bad resolve arguments (N=%d, %d columns per block)", p.N, BN);
  static ccx_lds_optin optin;
  if (lds > 64 * 1024) CCX_HIP(ctx, optin.ensure(ctx->device, (const void*)dec_linear_kernel<MT, NT, KMAX, ACT, EPI>));
  dim3 grid(ccx_cdiv(p.N, BN), ccx_cdiv(p.M, MROWS), ksplit);
  {
    // weight-streaming GEMV: algorithmic bytes = the weight matrix once (+ small activations)
    // labelled like rocprofv3 labels the instantiation, so that both rank the same kernels
    static const std::string label = "dec_linear_kernel<" + std::to_string(MT) + ", " + std::to_string(NT) + ", " + std::to_string(KMAX) +
                                     ", " + std::to_string(ACT) + ", " + std::to_string(EPI) + ">";
    ccx_prof_scope ps(ctx, stream, label.c_str(), 2.0 * p.M * (double)p.N * p.K,
                      2.0 * (double)p.N * p.K + 2.0 * p.M * ((double)p.K + p.N));
    hipLaunchKernelGGL((dec_linear_kernel<MT, NT, KMAX, ACT, EPI>), grid, dim3(256), lds, stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

template <int NT, int ACT, int EPI>
static int launch_dec_linear_mt(ccx_ctx* ctx, const DecLinearParams& p, int ksplit, hipStream_t stream) {
  const int M = p.M;
  // prefetch depth = k-steps per wave: 6 covers K = 768 (24 k-steps over 4 waves) without the two clamped duplicate
  // loads per fragment row and the 25 % idle registers of the depth-8 instantiation, which K = 1024 slices need
  const int need = ccx_cdiv(ccx_cdiv(p.K / 32, ksplit), 4);
  if (need <= 6) {
    if (M <= 16) return launch_dec_linear_inst<1, NT, 6, ACT, EPI>(ctx, p, ksplit, stream);
    if (M <= 32) return launch_dec_linear_inst<2, NT, 6, ACT, EPI>(ctx, p, ksplit, stream);
    return launch_dec_linear_inst<4, NT, 6, ACT, EPI>(ctx, p, ksplit, stream);
  }
  if (need <= 8) {
    if (M <= 16) return launch_dec_linear_inst<1, NT, 8, ACT, EPI>(ctx, p, ksplit, stream);
    if (M <= 32) return launch_dec_linear_inst<2, NT, 8, ACT, EPI>(ctx, p, ksplit, stream);
    return launch_dec_linear_inst<4, NT, 8, ACT, EPI>(ctx, p, ksplit, stream);
  }
  // depth 10: K = 1280 in one block (40 k-steps over 4 waves) and the 1280-wide slabs of K = 5120
  if (M <= 16) return launch_dec_linear_inst<1, NT, 10, ACT, EPI>(ctx, p, ksplit, stream);
  if (M <= 32) return launch_dec_linear_inst<2, NT, 10, ACT, EPI>(ctx, p, ksplit, stream);
  return launch_dec_linear_inst<4, NT, 10, ACT, EPI>(ctx, p, ksplit, stream);
}

int ccx_dec_packed_act_switch() {
  const char* e = getenv("CCX_DEC_PACKED_ACT");
  return !(e && strcmp(e, "0") == 0);
}

int ccx_dec_packed_mid_switch() {
  const char* e = getenv("CCX_DEC_PACKED_MID");
  return !(e && strcmp(e, "0") == 0);
}

int ccx_dec_linear_ksplit(int K, int epi) {
  // prefetch depth is 8 k-steps (256 elements) per wave, 4 waves per block -- or 10 (320 elements), taken only where 8 cannot serve:
  // a non-partial epilogue at 1024 < K <= 1280, and partial outputs whose 1024-wide slabs would outnumber the 4 pending slabs the
  // LayerNorm prologues fold in (K = 5120: 4 slabs of 1280 instead of 5 of 1024).  Everything up to K = 4096 splits as before.
  if (epi == DEPI_RESOLVE) return 1;   // the residual is added in place: one block owns all of K
  int ks = ccx_cdiv(K, 1024);
  if (epi != DEPI_PARTIAL) return K <= 1280 ? 1 : ks;  // only partial outputs can be split across blocks
  if (ks > 4) ks = ccx_cdiv(K, 1280);
  return ks < 1 ? 1 : ks;
}

int ccx_launch_dec_linear(ccx_ctx* ctx, int act, int epi, const DecLinearParams& p, hipStream_t stream) {
  CCX_REQUIRE(ctx, p.M > 0 && p.N > 0 && p.K > 0 && p.K % 32 == 0, "dec_linear: bad shape M=%d N=%d K=%d", p.M, p.N, p.K);
  CCX_REQUIRE(ctx, act == ACT_BF16 || p.K <= 1280, "dec_linear: LN/combine activation needs K <= 1280");
  CCX_REQUIRE(ctx, p.pend_n >= 0 && p.pend_n <= 4, "dec_linear: at most 4 pending slabs");
  CCX_REQUIRE(ctx, !p.act_packed || act == ACT_BF16, "dec_linear: act_packed is taken with bf16 activations only");
  CCX_REQUIRE(ctx, !p.out_packed || (act == ACT_BF16 && (epi == DEPI_BF16_GELU || epi == DEPI_RESOLVE) && p.N % 32 == 0),
              "dec_linear: out_packed needs the GELU or the resolve epilogue and N=%d a multiple of 32", p.N);
  const int ksplit = ccx_dec_linear_ksplit(p.K, epi);
  CCX_REQUIRE(ctx, epi == DEPI_PARTIAL || ksplit == 1, "dec_linear: K=%d needs a split-K (partial) epilogue", p.K);
  CCX_REQUIRE(ctx, ksplit <= 4, "dec_linear: K=%d would leave %d partial slabs (at most 4)", p.K, ksplit);
  CCX_REQUIRE(ctx, epi != DEPI_PARTIAL || p.pend_stride >= (long)p.M * p.ldo, "dec_linear: pend_stride too small");
  // Every wave of a block must own a k-step of its grid.z slice: a wave left without one (slices of 1, 2, 3, 5, 6 or 9 k-steps) still
  // issues its clamped weight and activation prefetch from ks0 = kz0 + wave * per_w, which then lies behind the slice -- for the
  // last column tile behind the packed weight image.  The model never asks for one: n_state is a multiple of 128, the MLP 4 x that.
  {
    int len = 0;
    const int z = ccx_dec_linear_starved_slice(p.K, ksplit, &len);
    CCX_REQUIRE(ctx, z < 0, "dec_linear: K=%d leaves K slice %d of %d with %d k-steps, too few for each of the 4 waves to own one", p.K, z, ksplit, len);
  }
  // Lanes of 128 rows and more (the decode groups of the pipelined schedule): a block of 16 output columns re-reads all of its 64
  // activation rows for 24 KB of weights, so the launch is bound by activation reads out of L2 (85 MB for the 1.2 MB QKV matrix
  // at 384 rows); 32 columns per block halve that: pipeline step 678.3 -> 653.8 ms with 2 lanes x 384 rows, 698 -> 683 with
  // 3 x 128 (64 columns per block: 659.9).  The in-place resolve of the X-stream path's out projection (DEPI_RESOLVE) follows
  // the same rule for every row count, so a row's numbers do not depend on its lane.
  if (epi == DEPI_RESOLVE) {
    CCX_REQUIRE(ctx, act == ACT_BF16, "dec_linear: the resolve epilogue takes bf16 activations");
    if (p.M >= 128) return launch_dec_linear_mt<2, ACT_BF16, DEPI_RESOLVE>(ctx, p, 1, stream);
    return launch_dec_linear_mt<1, ACT_BF16, DEPI_RESOLVE>(ctx, p, 1, stream);
  }
  if (p.M >= 128 && act == ACT_BF16) {
    if (epi == DEPI_PARTIAL) return launch_dec_linear_mt<2, ACT_BF16, DEPI_PARTIAL>(ctx, p, ksplit, stream);
    if (epi == DEPI_F32) return launch_dec_linear_mt<2, ACT_BF16, DEPI_F32>(ctx, p, 1, stream);
    if (epi == DEPI_SELF_QKV) return launch_dec_linear_mt<2, ACT_BF16, DEPI_SELF_QKV>(ctx, p, 1, stream);
    if (epi == DEPI_BF16_GELU) return launch_dec_linear_mt<2, ACT_BF16, DEPI_BF16_GELU>(ctx, p, 1, stream);
  }
  if (act == ACT_LN && epi == DEPI_SELF_QKV) return launch_dec_linear_mt<1, ACT_LN, DEPI_SELF_QKV>(ctx, p, 1, stream);
  if (act == ACT_LN && epi == DEPI_F32) return launch_dec_linear_mt<1, ACT_LN, DEPI_F32>(ctx, p, 1, stream);
  if (act == ACT_LN && epi == DEPI_BF16_GELU) return launch_dec_linear_mt<1, ACT_LN, DEPI_BF16_GELU>(ctx, p, 1, stream);
  if (act == ACT_COMBINE && epi == DEPI_PARTIAL) return launch_dec_linear_mt<1, ACT_COMBINE, DEPI_PARTIAL>(ctx, p, ksplit, stream);
  if (act == ACT_BF16 && epi == DEPI_PARTIAL) return launch_dec_linear_mt<1, ACT_BF16, DEPI_PARTIAL>(ctx, p, ksplit, stream);
  if (act == ACT_BF16 && epi == DEPI_F32) return launch_dec_linear_mt<1, ACT_BF16, DEPI_F32>(ctx, p, 1, stream);
  if (act == ACT_BF16 && epi == DEPI_SELF_QKV) return launch_dec_linear_mt<1, ACT_BF16, DEPI_SELF_QKV>(ctx, p, 1, stream);
  if (act == ACT_BF16 && epi == DEPI_BF16_GELU) return launch_dec_linear_mt<1, ACT_BF16, DEPI_BF16_GELU>(ctx, p, 1, stream);
  return ccx_fail(ctx, CCX_ERR_ARG, "dec_linear: unsupported act=%d epi=%d", act, epi);
}

// ------------------------------------------------------------------------------------------
// Single-query attention (self: T = pos+1 keys, FINAL output; cross: split-KV partials)
// ------------------------------------------------------------------------------------------
// The online-softmax core every attention kernel below is made of.  A wave instruction covers 8 keys x 128 B (lane group g = lane >> 3
// = key, c = lane & 7 = 16-byte d chunk), so a lane keeps the running state of ITS key residue and d chunk: the maximum m (log2
// domain), the sum l and the 8 output values o.  Lane groups merge in registers, waves through LDS.  Every kernel does the same
// floating-point operations in the same order here, which is what keeps the fused-query path bit-identical to the two-launch one.
struct SoftState {
  float m, l, o[8];
};
// (a function called where the kernels always set their state up, not default member initialisers: those move the SGPR counts of
//  the prefill kernels)
__device__ __forceinline__ void soft_init(SoftState& st) {
  st.m = -1e30f; st.l = 0.f;
#pragma unroll
  for (int j = 0; j < 8; j++) st.o[j] = 0.f;
}

__device__ __forceinline__ void load_q8(float (&q)[8], const float* src) {
  const float4 a = *(const float4*)src, d = *(const float4*)(src + 4);
  q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; q[4] = d.x; q[5] = d.y; q[6] = d.z; q[7] = d.w;
}

// Requests a piece of NIT x 8 keys of K and V from key `base` on, K first (the scores need it first).  Keys from `limit` on re-read
// row `last` (one cache line) instead of branching, and soft_update masks them.  NONTEMPORAL: the cross-attention K/V of a decode
// step is read exactly once (0.9 GB per layer and step); the prompt rows of a prefill share theirs through L2, so those loads stay
// cacheable.
template <int NIT, bool NONTEMPORAL>
__device__ __forceinline__ void kv_load(bf16x8 (&kf)[NIT], bf16x8 (&vf)[NIT], const bf16_t* Kb, const bf16_t* Vb, int base, int g,
                                        int limit, int last) {
  long off[NIT];
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    int key = base + it * 8 + g;
    key = key < limit ? key : last;
    off[it] = (long)key * 64;
  }
#pragma unroll
  for (int it = 0; it < NIT; it++) kf[it] = NONTEMPORAL ? __builtin_nontemporal_load((const bf16x8*)(Kb + off[it])) : *(const bf16x8*)(Kb + off[it]);
#pragma unroll
  for (int it = 0; it < NIT; it++) vf[it] = NONTEMPORAL ? __builtin_nontemporal_load((const bf16x8*)(Vb + off[it])) : *(const bf16x8*)(Vb + off[it]);
}

// Folds a piece of NIT x 8 keys into the state: scores q . k (log2 domain), -inf from key `limit` on, running maximum, rescale,
// accumulate p v.
template <int NIT>
__device__ __forceinline__ void soft_update(SoftState& st, const float (&q)[8], const bf16x8 (&kf)[NIT], const bf16x8 (&vf)[NIT],
                                            int base, int g, int limit, float scale_log2e) {
  float s[NIT];
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) a = fmaf(q[j], bf16_to_f32((bf16_t)kf[it][j]), a);
    a = group8_sum(a) * scale_log2e;
    s[it] = (base + it * 8 + g < limit) ? a : -INFINITY;
  }
  float mn = st.m;
#pragma unroll
  for (int it = 0; it < NIT; it++) mn = fmaxf(mn, s[it]);
  const float al = __builtin_amdgcn_exp2f(st.m - mn);
  st.l *= al;
#pragma unroll
  for (int j = 0; j < 8; j++) st.o[j] *= al;
#pragma unroll
  for (int it = 0; it < NIT; it++) {
    const float pe = __builtin_amdgcn_exp2f(s[it] - mn);
    st.l += pe;
#pragma unroll
    for (int j = 0; j < 8; j++) st.o[j] = fmaf(pe, bf16_to_f32((bf16_t)vf[it][j]), st.o[j]);
  }
  st.m = mn;
}

// state a takes in (bm, bl, bo).  Of x * wa + y * wb an fma can take either product, and the two round differently; left to the
// compiler the pick depends on the code around the merge.  PINNED: fma(bo, wb, a.o * wa) written out -- what the kernels must
// share (fused-query and two-launch partials agree bit for bit).  PINNED = false leaves the text to the compiler, see below.
template <bool PINNED = true>
__device__ __forceinline__ void soft_merge(SoftState& a, float bm, float bl, const float (&bo)[8]) {
  const float mx = fmaxf(a.m, bm);
  const float wa = __builtin_amdgcn_exp2f(a.m - mx), wb = __builtin_amdgcn_exp2f(bm - mx);
  a.l = a.l * wa + bl * wb;
#pragma unroll
  for (int j = 0; j < 8; j++) a.o[j] = PINNED ? fmaf(bo[j], wb, a.o[j] * wa) : a.o[j] * wa + bo[j] * wb;
  a.m = mx;
}

// merge the 8 lane groups (lanes with equal c) in registers: xor 8 via DPP row_ror:8, xor 16 /
// xor 32 via v_permlane16_swap / v_permlane32_swap (VALU speed, no LDS round trips).
// PINNED = false (dec_cross_prefill_kernel only): its xor 16 and xor 32 merges have always come out of the compiler fused the other
// way, fma(a.o, wa, bo * wb).  Writing that out moves the kernel's registers and its s_waitcnt sequence, so there the text stays
// unpinned and a prompt's numbers stay what they were.
template <bool PINNED = true>
__device__ __forceinline__ void soft_merge_lane_groups(SoftState& st) {
  float om, ol, oo[8];
  om = dpp_mov<0x128>(st.m); ol = dpp_mov<0x128>(st.l);
#pragma unroll
  for (int j = 0; j < 8; j++) oo[j] = dpp_mov<0x128>(st.o[j]);
  soft_merge(st, om, ol, oo);
  om = lane_xor16(st.m); ol = lane_xor16(st.l);
#pragma unroll
  for (int j = 0; j < 8; j++) oo[j] = lane_xor16(st.o[j]);
  soft_merge<PINNED>(st, om, ol, oo);
  om = lane_xor32(st.m); ol = lane_xor32(st.l);
#pragma unroll
  for (int j = 0; j < 8; j++) oo[j] = lane_xor32(st.o[j]);
  soft_merge<PINNED>(st, om, ol, oo);
}

// The four waves of a block meet in LDS: lane group 0 of every wave stores its merged state (the caller puts the barrier between
// the two), then the thread that owns output d = 8 cc + j merges the waves in the order w = 0..3.
__device__ __forceinline__ void soft_store_wave(float (&sm_m)[4][8], float (&sm_l)[4][8], float (&sm_o)[4][8][8], const SoftState& st,
                                                int wave, int g, int c) {
  if (g == 0) {
    sm_m[wave][c] = st.m; sm_l[wave][c] = st.l;
#pragma unroll
    for (int j = 0; j < 8; j++) sm_o[wave][c][j] = st.o[j];
  }
}
__device__ __forceinline__ void soft_merge_waves(const float (&sm_m)[4][8], const float (&sm_l)[4][8], const float (&sm_o)[4][8][8], int d,
                                                 float& mx, float& l, float& o) {
  const int cc = d >> 3, j = d & 7;
  mx = fmaxf(fmaxf(sm_m[0][cc], sm_m[1][cc]), fmaxf(sm_m[2][cc], sm_m[3][cc]));
  l = 0.f; o = 0.f;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const float ww = __builtin_amdgcn_exp2f(sm_m[w][cc] - mx);
    l += ww * sm_l[w][cc];
    o += ww * sm_o[w][cc][j];
  }
}

// A wave owns 64-key chunks and issues all 16 K/V loads of a chunk before touching the data, so one
// HBM round trip covers the chunk.
// IND (beam search, self attention only): key t of row b is read from cache slot ind[b][t] instead of slot sq -- a hypothesis that moved
// to another row keeps reading the K/V its ancestors wrote, no cache row is ever copied.  A chunk's 8 slot entries are requested
// before any of its K/V loads (they are the head of a dependent chain: one more round trip per 64-key chunk, out of L2).  The
// unflagged instantiations are the kernels they always were.
// IMG (FINAL self attention of a decode step, DecAttnParams::out_packed): the output rows are written as the fragment image the out
// projection loads (decoder.h dec_frag_off) instead of row-major.  A compile-time flag: the other instantiations' code does not change.
template <bool FINAL, bool IND = false, bool IMG = false>
__global__ __launch_bounds__(256) void dec_attention_kernel(DecAttnParams p) {
  __shared__ float sm_m[4][8], sm_l[4][8], sm_o[4][8][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, split = blockIdx.y;
  const int b = bh / p.H, h = bh - b * p.H;        // b: row (q / out); its K/V belong to sequence sq
  const int sq = p.row_seq ? p.row_seq[b] : b;
  const int g = lane >> 3, c = lane & 7;
  const int T = p.pos ? (p.pos[b] + 1) : p.T;
  const int per = (T + gridDim.y - 1) / gridDim.y;
  const int kbeg = split * per;
  const int kend = (kbeg + per < T) ? kbeg + per : T;

  const bf16_t* Kb = p.k + ((long)sq * p.H + h) * p.kv_T * 64 + 8 * c;
  const bf16_t* Vb = p.v + ((long)sq * p.H + h) * p.kv_T * 64 + 8 * c;

  SoftState st;
  soft_init(st);
  float q[8];
  load_q8(q, p.q + ((long)b * p.H + h) * 64 + 8 * c);

  for (int base = kbeg + wave * 64; base < kend; base += 256) {
    bf16x8 kf[8], vf[8];
    if (IND) {
      const unsigned short* ir = p.ind + (long)b * p.ind_ld;
      const bf16_t* K0 = p.k + 8 * c;
      const bf16_t* V0 = p.v + 8 * c;
      int key[8]; unsigned slot[8];
#pragma unroll
      for (int it = 0; it < 8; it++) {
        key[it] = base + it * 8 + g;
        key[it] = key[it] < kend ? key[it] : kend - 1;
        slot[it] = ir[key[it]];
      }
#pragma unroll
      for (int it = 0; it < 8; it++) {
        const long off = (((long)slot[it] * p.H + h) * p.kv_T + key[it]) * 64;
        kf[it] = *(const bf16x8*)(K0 + off);
        vf[it] = *(const bf16x8*)(V0 + off);
      }
      soft_update<8>(st, q, kf, vf, base, g, kend, p.scale_log2e);
      continue;
    }
    // (not kv_load: its K-first order costs this kernel a VGPR less and other SGPRs, and its register figures are pinned)
#pragma unroll
    for (int it = 0; it < 8; it++) {
      int key = base + it * 8 + g;
      key = key < kend ? key : kend - 1;
      if (FINAL) {   // self attention: the cache rows were written moments ago, keep them cacheable
        kf[it] = *(const bf16x8*)(Kb + (long)key * 64);
        vf[it] = *(const bf16x8*)(Vb + (long)key * 64);
      } else {       // cross attention: 0.9 GB per layer and step, read exactly once -> non-temporal
        kf[it] = __builtin_nontemporal_load((const bf16x8*)(Kb + (long)key * 64));
        vf[it] = __builtin_nontemporal_load((const bf16x8*)(Vb + (long)key * 64));
      }
    }
    soft_update<8>(st, q, kf, vf, base, g, kend, p.scale_log2e);
  }
  soft_merge_lane_groups(st);
  soft_store_wave(sm_m, sm_l, sm_o, st, wave, g, c);
  __syncthreads();
  if (tid < 64) {
    float mx, l, o;
    soft_merge_waves(sm_m, sm_l, sm_o, tid, mx, l, o);
    if (FINAL) {
      p.out_bf16[IMG ? dec_frag_off(b, h * 64 + tid, p.H * 2) : ((long)b * p.H + h) * 64 + tid] = f32_to_bf16(o / l);
    } else {
      const long pbase = ((long)b * p.H + h) * gridDim.y + split;
      p.part_o[pbase * 64 + tid] = o;
      if (tid == 0) { p.part_ml[pbase * 2] = mx; p.part_ml[pbase * 2 + 1] = l; }
    }
  }
}

// Small-batch cross attention with the query projection inside (B <= 16 rows: the reference's own calling pattern, one file per task
// and one window per decode, back/api.py:1286-1292).  The decode chain of a small batch is a string of latency-bound launches
// (~5-7 us each against a ~1 us HBM floor); this removes one of the eight per layer.  A block = (row, head, key split) as in
// dec_attention_kernel<false>; before it touches q it
//   1. requests its FIRST 64-key chunk of K and V (they do not depend on q: one HBM round trip now runs under the prologue),
//   2. requests the 4 x 6 weight fragments of its head's 64 query columns (wave w: k-steps 6 w .. 6 w + 5, the slice the same wave
//      of dec_linear_kernel<1, 1, 6, ACT_LN, DEPI_F32> owns),
//   3. normalises its row (every wave for itself into its own LDS row: no barrier) with the shared ln_* pieces,
//   4. runs the same 24 MFMAs, reduces the four waves' partial sums in the same order (w = 0..3) and adds the bias.
// Steps 3-4 repeat dec_linear's operations one for one, so q -- and with it every token and log-probability -- is bit-identical
// to the two-launch path (tests/test_whisper_gpu.py::test_fused_cross_query_equals_two_launches).  K == 768 only (24 k-steps).
// Register budget.  EARLY_V = false: <= 168 VGPRs (three blocks per CU, so that the 576 blocks of 8 rows x 12 heads x 6 splits are all
// resident): the K chunk (32) and two weight groups (64) are in flight across the LayerNorm (64) and the V chunk is requested only when
// the first MFMAs have freed a weight group -- its HBM round trip is then partly exposed.  EARLY_V = true (grids of <= 512 blocks, i.e.
// up to 7 rows: two blocks per CU hold them all): V is requested right behind K, 32 registers more.
template <bool EARLY_V>
__global__ __launch_bounds__(256, EARLY_V ? 2 : 3) void dec_cross_fused_q_kernel(DecAttnParams p) {
  __shared__ float sm_m[4][8], sm_l[4][8], sm_o[4][8][8];
  __shared__ __attribute__((aligned(16))) bf16_t ln_row[4][776];
  __shared__ __attribute__((aligned(16))) float red[4][4][4][4];     // [wave][n-tile][lane >> 4][4 outputs]: column 0 of every tile
  __shared__ __attribute__((aligned(16))) float q_s[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, split = blockIdx.y;
  const int b = bh / p.H, h = bh - b * p.H;
  const int g = lane >> 3, c = lane & 7;
  const int T = p.T;
  const int per = (T + gridDim.y - 1) / gridDim.y;
  const int kbeg = split * per;
  const int kend = (kbeg + per < T) ? kbeg + per : T;
  const int K = p.q_K;                       // 768
  // block-uniform bases + 32-bit byte offsets per lane (one SGPR pair + one VGPR per address instead of a 64-bit VGPR pair), which is
  // why this kernel has a chunk loader of its own instead of kv_load: 64 keys of K, of V or of both, clamped like kv_load (a wave
  // without keys loads row kend - 1 and soft_update masks it)
  const char* Ku = (const char*)(p.k + ((long)b * p.H + h) * p.kv_T * 64);
  const char* Vu = (const char*)(p.v + ((long)b * p.H + h) * p.kv_T * 64);
  bf16x8 kf[8], vf[8];
  auto load_chunk = [&](int base, bool want_k, bool want_v) {
#pragma unroll
    for (int it = 0; it < 8; it++) {
      int key = base + it * 8 + g;
      key = key < kend ? key : kend - 1;
      const unsigned off = (unsigned)(key * 64 + 8 * c) * 2u;
      if (want_k) kf[it] = __builtin_nontemporal_load((const bf16x8*)(Ku + off));
      if (want_v) vf[it] = __builtin_nontemporal_load((const bf16x8*)(Vu + off));
    }
  };

  // vmcnt retires IN ORDER, so whatever the LayerNorm waits for must be requested BEFORE the long HBM round trip of the K chunk:
  // ---- 1. the row, its pending split-K slabs and the LayerNorm's affine parameters (L2 hits) ----
  const int nv = K >> 2;
  const long row = (long)b * K;
  float4 v[4], pq[4], gg[4], bb[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int idx = lane + 64 * i;
    const int ic = idx < nv ? idx : 0;
    const unsigned o16 = (unsigned)ic * 16u;
    v[i] = *(const float4*)((const char*)(p.qx + row) + o16);
    // (dec_linear adds all four slab slots, the unused ones with weight 0: fmaf(0, finite, a) == a, so skipping them is bit-identical;
    //  two or more pending slabs take the generic loop below)
    pq[i] = *(const float4*)((const char*)(p.q_pend + row) + o16);
    gg[i] = *(const float4*)((const char*)p.q_ln_g + o16);
    bb[i] = *(const float4*)((const char*)p.q_ln_b + o16);
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- 2. first K chunk of this wave ----
  load_chunk(kbeg + wave * 64, true, EARLY_V);
  // ---- 3. weight fragments: n-tiles 4 h .. 4 h + 3, k-steps 6 wave .. 6 wave + 5 (packed image: tile (n / 16, k / 32) = 1 KB), in three
  // groups of two k-steps (32 registers each, at most two groups in flight).  Default cache policy: the 48 blocks of a head share them.
  const int ksteps = K >> 5;                 // 24
  const int ks0 = wave * 6;
  const char* wu = (const char*)(p.q_W + ((long)(4 * h) * ksteps + ks0) * 512);       // block- and wave-uniform
  auto load_group = [&](int gk, bf16x8 (&w)[4][2]) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int k = 0; k < 2; k++) w[i][k] = *(const bf16x8*)(wu + (unsigned)(((i * ksteps + 2 * gk + k) * 64 + lane) * 16));
  };
  bf16x8 wa[4][2], wb[4][2];
  load_group(0, wa);
  __builtin_amdgcn_sched_barrier(0);
  // ---- 4. LayerNorm of row b (x + pending slabs), every wave for itself ----
  {
    const bool writer = (h == 0 && split == 0 && wave == 0 && p.q_x_out != nullptr);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int idx = lane + 64 * i;
      const int ic = idx < nv ? idx : 0;
      float4 a = v[i];
      a = ln_add_pend(a, p.q_pend_n > 0 ? 1.f : 0.f, pq[i]);
      for (int s = 1; s < p.q_pend_n; s++)       // (rare: only K > 1024 producers leave more than one slab)
        a = ln_add_pend(a, 1.f, ((const float4*)(p.q_pend + (long)s * p.q_pend_stride + row))[ic]);
      if (idx >= nv) a = make_float4(0.f, 0.f, 0.f, 0.f);
      v[i] = a;
    }
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) sm += ln_sum4(v[i]);
    const float mean = wave_reduce_sum(sm) / (float)K;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float t = ln_sq4(v[i], mean);
      sq += (lane + 64 * i < nv) ? t : 0.f;
    }
    const float rstd = rsqrtf(wave_reduce_sum(sq) / (float)K + p.q_eps);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int idx = lane + 64 * i;
      if (idx < nv) {
        *(uint2*)(&ln_row[wave][4 * idx]) = ln_pack4(v[i], mean, rstd, gg[i], bb[i]);
        if (writer) ((float4*)(p.q_x_out + row))[idx] = v[i];
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  load_group(1, wb);
  // the wave's own LDS row: its stores are complete once lgkmcnt is 0, no other wave reads it
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // ---- 5. q = row * Wq^T: the activation fragment is the same row in every MFMA column; k-steps in the order 0..5 ----
  float4 bias4;
  {
    const int h4 = lane >> 4;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto mma_group = [&](int gk, const bf16x8 (&w)[4][2]) {
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const bf16x8 af = *(const bf16x8*)(&ln_row[wave][8 * h4 + 32 * (ks0 + 2 * gk + k)]);
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[i][k], af, acc[i], 0, 0, 0);
      }
    };
    mma_group(0, wa);
    __builtin_amdgcn_sched_barrier(0);
    load_group(2, wa);
    bias4 = *(const float4*)(p.q_bias + h * 64 + 4 * (tid & 15));     // (no branch around the load: hipcc would wait at it)
    // first V chunk behind the last weight group (its HBM round trip runs under the remaining MFMAs, the reduction and q . k)
    if (!EARLY_V) load_chunk(kbeg + wave * 64, false, true);
    __builtin_amdgcn_sched_barrier(0);
    mma_group(1, wb);
    mma_group(2, wa);
    if ((lane & 15) == 0) {
#pragma unroll
      for (int i = 0; i < 4; i++) *(f32x4*)(&red[wave][i][h4][0]) = acc[i];
    }
  }
  __syncthreads();
  if (tid < 16) {
    // thread t finishes outputs 4 t .. 4 t + 3 of the head: n-tile t >> 2, rows 4 (t & 3) .. + 3; waves summed in the order 0..3
    const int i = tid >> 2, r4 = tid & 3;
    f32x4 v = *(const f32x4*)(&red[0][i][r4][0]);
#pragma unroll
    for (int w = 1; w < 4; w++) v += *(const f32x4*)(&red[w][i][r4][0]);
    v[0] += bias4.x; v[1] += bias4.y; v[2] += bias4.z; v[3] += bias4.w;
    *(float4*)(&q_s[4 * tid]) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  float q[8];
  load_q8(q, &q_s[8 * c]);

  // ---- attention over this block's keys: dec_attention_kernel<false>'s loop (the same soft_* calls, so the same partials bit for
  // bit), its first chunk already in registers ----
  SoftState st;
  soft_init(st);
  for (int base = kbeg + wave * 64; base < kend; base += 256) {
    if (base != kbeg + wave * 64) load_chunk(base, true, true);
    soft_update<8>(st, q, kf, vf, base, g, kend, p.scale_log2e);
  }
  soft_merge_lane_groups(st);
  soft_store_wave(sm_m, sm_l, sm_o, st, wave, g, c);
  __syncthreads();
  if (tid < 64) {
    float mx, l, o;
    soft_merge_waves(sm_m, sm_l, sm_o, tid, mx, l, o);
    const long pbase = ((long)b * p.H + h) * gridDim.y + split;
    p.part_o[pbase * 64 + tid] = o;
    if (tid == 0) { p.part_ml[pbase * 2] = mx; p.part_ml[pbase * 2 + 1] = l; }
  }
}

int ccx_launch_dec_cross_fused_q(ccx_ctx* ctx, const DecAttnParams& p, int B, int nsplit, hipStream_t stream) {
  CCX_REQUIRE(ctx, B > 0 && B <= 16 && p.H > 0 && nsplit >= 1 && nsplit <= 8, "dec_cross_fused_q: bad shape");
  CCX_REQUIRE(ctx, p.q_K == 768 && p.H * 64 == p.q_K && !p.pos && !p.row_seq, "dec_cross_fused_q: needs d_model 768 and one row per sequence");
  CCX_REQUIRE(ctx, p.qx && p.q_W && p.q_bias && p.q_ln_g && p.q_ln_b && p.q_pend && p.q_pend_n >= 0 && p.q_pend_n <= 4, "dec_cross_fused_q: missing operands");
  CCX_REQUIRE(ctx, p.q_x_out != p.qx, "dec_cross_fused_q: x_out must not alias x");
  {
    // algorithmic bytes: the K/V of the batch once + the query weights once
    ccx_prof_scope ps(ctx, stream, "dec_cross_fused_q_kernel", 4.0 * B * p.H * (double)p.T * 64 + 2.0 * B * (double)p.q_K * p.q_K,
                      (double)B * p.H * p.T * 64 * 2 * 2 + 2.0 * p.q_K * p.q_K);
    if (B * p.H * nsplit <= 512) hipLaunchKernelGGL(dec_cross_fused_q_kernel<true>, dim3(B * p.H, nsplit), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(dec_cross_fused_q_kernel<false>, dim3(B * p.H, nsplit), dim3(256), 0, stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// Cross attention for decode lanes that overlap other lanes' latency-bound chains ("lean streaming").  The chain kernels of
// the other lanes are slowed mostly by the memory queue of the CU they share with streaming waves (MI355X_MICROARCH.md,
// handoff-1to1: 0.8 us idle, 2.3-2.8 us beside 8 streaming waves, 1.2-1.5 beside 2-5), so this variant keeps FEW waves per CU
// and FEW bytes per wave in flight while still covering HBM latency: a wave owns one contiguous key range and rolls through it
// in 32-key pieces (4 K + 4 V wave loads = 8 KB), the next piece always requested before the current one is reduced
// (two named register sets; hipcc leaves the younger 8 loads in flight: s_waitcnt vmcnt(8)).
// NP = 32-key pieces per wave (compile-time: the loop is fully unrolled into straight-line code, because with a real loop
// hipcc keeps the loop-carried piece in other registers than it loads into and copies it at the loop end behind a vmcnt(0)).
// PRE (prompt prefill): a sequence has rows_per_seq consecutive rows (one per prompt position) that all attend to ITS K/V.  Logical
// block L = (sequence * H + head) * rows_per_seq + t, and the launch order is remapped (xcd_remap, the GEMM's map) so
// that the rows of one (sequence, head) run on one XCD at about the same time: the first one brings the 384 KB of K/V into
// that XCD's L2, the others hit it -- the prompt costs about one step of HBM traffic instead of one per prompt token.  Loads are
// cacheable here (non-temporal for the decode steps, where every byte is used once).
// MAP (a decode over a row -> window map, ccx_whisper_decode_rows): the K/V of a row are those of sequence row_seq[row] -- entries may
// repeat, need not be monotone and may leave sequences unused; q and out stay indexed by the row.  PRE && MAP: the rows of group `sq`
// read the sequence row_seq[sq * rows_per_seq] (the host composes the prefill's row table with the map).  One scalar load per block on
// top of the unmapped kernel; MAP = false is that kernel, instruction for instruction.
template <bool FINAL, int NP, bool PRE = false, bool MAP = false>
__global__ __launch_bounds__(256) void dec_cross_stream_kernel(DecAttnParams p) {
  static_assert(FINAL, "one block owns the whole key range of a (row, head): final output, no split-KV partials");
  __shared__ float sm_m[4][8], sm_l[4][8], sm_o[4][8][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.y;
  int b, h, sq;                                      // row (q / out), head, sequence (K/V)
  if (PRE) {
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int t = L % p.rows_per_seq, sh = L / p.rows_per_seq;
    h = sh % p.H; sq = sh / p.H;
    b = sq * p.rows_per_seq + t;
  } else {
    const int bh = blockIdx.x;
    b = bh / p.H; h = bh - b * p.H; sq = b;
  }
  const int kvs = MAP ? __builtin_amdgcn_readfirstlane(p.row_seq[PRE ? sq * p.rows_per_seq : b]) : sq;   // sequence of the K/V
  const int g = lane >> 3, c = lane & 7;
  const int T = p.T;
  const int per = (T + gridDim.y - 1) / gridDim.y;
  const int kbeg = split * per;
  const int kend = (kbeg + per < T) ? kbeg + per : T;
  // contiguous range of this wave, in multiples of 32 keys
  const int per_w = (((kend - kbeg) + 3) / 4 + 31) & ~31;
  // wave-uniform by construction; readfirstlane makes it provable, so the loop below branches on scalars (s_cbranch_scc)
  // instead of masking lanes, and hipcc can count its loads (vmcnt(8)) instead of draining them
  // (the four waves taking alternating pieces of ONE sweep over the block's keys instead of a contiguous quarter each was
  // measured too: 92.2 against 93.7 us per launch alone, 706.0 against 704.4 ms per pipeline step -- no difference)
  const int w0 = __builtin_amdgcn_readfirstlane(kbeg + wave * per_w);
  const int w1 = __builtin_amdgcn_readfirstlane((w0 + per_w < kend) ? w0 + per_w : kend);
  constexpr int PSTEP = 32;

  const bf16_t* Kb = p.k + ((long)kvs * p.H + h) * p.kv_T * 64 + 8 * c;
  const bf16_t* Vb = p.v + ((long)kvs * p.H + h) * p.kv_T * 64 + 8 * c;

  SoftState st;   // set up in place: through soft_init() the PRE instantiations' SGPR counts move by one, and the register figures are pinned
  st.m = -1e30f; st.l = 0.f;
#pragma unroll
  for (int j = 0; j < 8; j++) st.o[j] = 0.f;
  float q[8];
  load_q8(q, p.q + ((long)b * p.H + h) * 64 + 8 * c);
  auto load = [&](bf16x8 (&kf)[4], bf16x8 (&vf)[4], int base) { kv_load<4, !PRE>(kf, vf, Kb, Vb, base, g, w1, kend - 1); };
  auto reduce = [&](const bf16x8 (&kf)[4], const bf16x8 (&vf)[4], int base) { soft_update<4>(st, q, kf, vf, base, g, w1, p.scale_log2e); };
  {
    // no branch around a request or a reduce: one code path, exact load counts.  Pieces past the end of the wave's range
    // re-read its last key row (one cache line) and are masked to -inf scores.  sched_barrier pins the order
    // request(i+1) -> reduce(i): at most two pieces (16 KB) and at least one (8 KB) in flight per wave.
    bf16x8 kA[4], vA[4], kB[4], vB[4];
    load(kA, vA, w0);
    // q is consumed once HERE: behind the first piece's requests, so that its round trip and theirs overlap (the wait is a
    // counted vmcnt(8): q is older than the piece), and before the loop (a wait for q inside it would sit on every iteration)
    __builtin_amdgcn_sched_barrier(0);
    {
      float qs = 0.f;
#pragma unroll
      for (int j = 0; j < 8; j++) qs += q[j];
      asm volatile("" ::"v"(qs));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NP; i += 2) {
      const int base = w0 + PSTEP * i;
      if (i + 1 < NP) load(kB, vB, base + PSTEP);
      __builtin_amdgcn_sched_barrier(0);
      reduce(kA, vA, base);
      __builtin_amdgcn_sched_barrier(0);
      if (i + 2 < NP) load(kA, vA, base + 2 * PSTEP);
      __builtin_amdgcn_sched_barrier(0);
      if (i + 1 < NP) reduce(kB, vB, base + PSTEP);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  soft_merge_lane_groups(st);
  soft_store_wave(sm_m, sm_l, sm_o, st, wave, g, c);
  __syncthreads();
  if (tid < 64) {
    float mx, l, o;
    soft_merge_waves(sm_m, sm_l, sm_o, tid, mx, l, o);
    p.out_bf16[((long)b * p.H + h) * 64 + tid] = f32_to_bf16(o / l);
  }
}

// Prompt prefill of the cross attention, RB prompt rows per block.  A sequence's prompt rows all attend to ITS K/V: with one block
// per (sequence, head, row) (dec_cross_stream_kernel<.., PRE>) the 384 KB of a head came out of L2 once per row (35 GB per
// 768-sequence prefill at 10 rows, ~2 TB/s effective).  Here a block streams the K/V of one (sequence, head) ONCE per RB rows:
// every 32-key piece is reduced against RB queries.  Same wave / piece structure as the streaming kernel (a wave owns a contiguous
// quarter of the keys, the next piece is requested before the current one is reduced), cacheable loads, XCD-aware block order.
template <int NP, int RB, bool MAP = false>
__global__ __launch_bounds__(256) void dec_cross_prefill_kernel(DecAttnParams p) {
  __shared__ float sm_m[RB][4][8], sm_l[RB][4][8], sm_o[RB][4][8][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ngrp = (p.rows_per_seq + RB - 1) / RB;                  // row groups per (sequence, head)
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int tg = L % ngrp, sh = L / ngrp;
  const int h = sh % p.H, sq = sh / p.H;
  const int t0 = tg * RB;
  const int g = lane >> 3, c = lane & 7;
  const int T = p.T;
  const int per_w = ((T + 3) / 4 + 31) & ~31;
  const int w0 = __builtin_amdgcn_readfirstlane(wave * per_w);
  const int w1 = __builtin_amdgcn_readfirstlane((w0 + per_w < T) ? w0 + per_w : T);
  const int kvs = MAP ? __builtin_amdgcn_readfirstlane(p.row_seq[sq * p.rows_per_seq]) : sq;   // MAP: as dec_cross_stream_kernel
  const bf16_t* Kb = p.k + ((long)kvs * p.H + h) * p.kv_T * 64 + 8 * c;
  const bf16_t* Vb = p.v + ((long)kvs * p.H + h) * p.kv_T * 64 + 8 * c;

  float q[RB][8];
  SoftState st[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) {
    const int t = t0 + r < p.rows_per_seq ? t0 + r : p.rows_per_seq - 1;      // rows past the prompt repeat the last one (not stored)
    load_q8(q[r], p.q + ((long)(sq * p.rows_per_seq + t) * p.H + h) * 64 + 8 * c);
    soft_init(st[r]);
  }
  auto load = [&](bf16x8 (&kf)[4], bf16x8 (&vf)[4], int base) { kv_load<4, false>(kf, vf, Kb, Vb, base, g, w1, T - 1); };
  {
    // a real loop here (the decode-step kernel is straight-line code for exact load counts; this one runs once per decode
    // and lives within 256 registers only as a loop): the next piece is requested, the current one reduced against RB rows
    bf16x8 kA[4], vA[4], kB[4], vB[4];
    load(kA, vA, w0);
#pragma unroll 1
    for (int i = 0; i < NP; i++) {
      const int base = w0 + 32 * i;
      load(kB, vB, base + 32 < w1 ? base + 32 : base);
#pragma unroll
      for (int r = 0; r < RB; r++) soft_update<4>(st[r], q[r], kA, vA, base, g, w1, p.scale_log2e);
#pragma unroll
      for (int it = 0; it < 4; it++) { kA[it] = kB[it]; vA[it] = vB[it]; }
    }
  }
#pragma unroll
  for (int r = 0; r < RB; r++) {
    soft_merge_lane_groups<false>(st[r]);
    soft_store_wave(sm_m[r], sm_l[r], sm_o[r], st[r], wave, g, c);
  }
  __syncthreads();
  for (int e = tid; e < RB * 64; e += 256) {
    const int r = e >> 6, d = e & 63;
    if (t0 + r >= p.rows_per_seq) continue;
    float mx, l, o;
    soft_merge_waves(sm_m[r], sm_l[r], sm_o[r], d, mx, l, o);
    p.out_bf16[((long)(sq * p.rows_per_seq + t0 + r) * p.H + h) * 64 + d] = f32_to_bf16(o / l);
  }
}

// One instantiation the launcher below can pick.  label = the symbol that runs (rocprofv3's kernel trace shows the same name), self
// attention marked as such; optin = its opt-in to static + dynamic LDS beyond 64 KB, for the forms that take lds_pad.
struct DecAttnKernel {
  const char* label;
  void (*fn)(DecAttnParams);
  ccx_lds_optin optin;
};

int ccx_launch_dec_attention(ccx_ctx* ctx, const DecAttnParams& p, int B, int nsplit, bool final_out,
                             hipStream_t stream) {
  CCX_REQUIRE(ctx, B > 0 && p.H > 0 && nsplit >= 1, "dec_attention: bad shape");
  CCX_REQUIRE(ctx, !final_out || nsplit == 1, "dec_attention: final output needs nsplit == 1");
  // the streaming and prefill instantiations by pieces per wave: keys per block / 4 waves, rounded up to 32 (the kernels' own formula)
  static DecAttnKernel prefill4[3] = {{"dec_cross_prefill_kernel<4,4>", dec_cross_prefill_kernel<4, 4>},
                                      {"dec_cross_prefill_kernel<6,4>", dec_cross_prefill_kernel<6, 4>},
                                      {"dec_cross_prefill_kernel<12,4>", dec_cross_prefill_kernel<12, 4>}};
  static DecAttnKernel prefill1[3] = {{"dec_cross_stream_kernel<true,4,true>", dec_cross_stream_kernel<true, 4, true>},
                                      {"dec_cross_stream_kernel<true,6,true>", dec_cross_stream_kernel<true, 6, true>},
                                      {"dec_cross_stream_kernel<true,12,true>", dec_cross_stream_kernel<true, 12, true>}};
  static DecAttnKernel streaming[3] = {{"dec_cross_stream_kernel<true,4,false>", dec_cross_stream_kernel<true, 4>},
                                       {"dec_cross_stream_kernel<true,6,false>", dec_cross_stream_kernel<true, 6>},
                                       {"dec_cross_stream_kernel<true,12,false>", dec_cross_stream_kernel<true, 12>}};
  // the same three over a row -> window map (DecAttnParams::kv_map)
  static DecAttnKernel prefill4_map[3] = {{"dec_cross_prefill_kernel<4,4,true>", dec_cross_prefill_kernel<4, 4, true>},
                                          {"dec_cross_prefill_kernel<6,4,true>", dec_cross_prefill_kernel<6, 4, true>},
                                          {"dec_cross_prefill_kernel<12,4,true>", dec_cross_prefill_kernel<12, 4, true>}};
  static DecAttnKernel prefill1_map[3] = {{"dec_cross_stream_kernel<true,4,true,true>", dec_cross_stream_kernel<true, 4, true, true>},
                                          {"dec_cross_stream_kernel<true,6,true,true>", dec_cross_stream_kernel<true, 6, true, true>},
                                          {"dec_cross_stream_kernel<true,12,true,true>", dec_cross_stream_kernel<true, 12, true, true>}};
  static DecAttnKernel streaming_map[3] = {{"dec_cross_stream_kernel<true,4,false,true>", dec_cross_stream_kernel<true, 4, false, true>},
                                           {"dec_cross_stream_kernel<true,6,false,true>", dec_cross_stream_kernel<true, 6, false, true>},
                                           {"dec_cross_stream_kernel<true,12,false,true>", dec_cross_stream_kernel<true, 12, false, true>}};
  static DecAttnKernel split_kv[2][2] = {   // [self][final]
      {{"dec_attention_kernel<false> (cross)", dec_attention_kernel<false>}, {"dec_attention_kernel<true> (cross)", dec_attention_kernel<true>}},
      {{"dec_attention_kernel<false> (self)", dec_attention_kernel<false>}, {"dec_attention_kernel<true> (self)", dec_attention_kernel<true>}}};
  // the image is written by the self attention of a decode step only: every other form would drop the flag or ignore it
  CCX_REQUIRE(ctx, !p.out_packed || (p.pos && final_out && nsplit == 1 && !p.row_seq && !p.ind && !p.stream_mode && p.rows_per_seq <= 1 && B % 16 == 0),
              "dec_attention: out_packed is taken by the self attention of a decode step (pos, nsplit 1, no row_seq, no ind) over whole 16-row tiles only (B=%d, nsplit=%d)", B, nsplit);
  const int np_need = p.pos ? 0 : ((ccx_cdiv(ccx_cdiv(p.T, nsplit), 4) + 31) / 32);
  const int npi = np_need <= 4 ? 0 : (np_need <= 6 ? 1 : 2);
  const bool prefill = p.rows_per_seq > 1 && !p.pos;
  const int pad = p.lds_pad > 0 ? (p.lds_pad < 128 * 1024 ? p.lds_pad : 128 * 1024) : 0;

  DecAttnKernel* k;
  dim3 grid(B * p.H, nsplit);
  int lds = 0;
  if (prefill) {
    // prompt prefill: B = sequences here, whole key range per block.  Three rows and more: four prompt rows per block (the K/V of
    // a (sequence, head) comes out of L2 once per four rows), else one block per (sequence, head, prompt row)
    CCX_REQUIRE(ctx, nsplit == 1 && final_out && np_need <= 12, "dec_attention: the prefill cross attention takes the whole key range (T <= 1536)");
    CCX_REQUIRE(ctx, !p.kv_map || p.row_seq, "dec_attention: kv_map needs row_seq");
    if (p.kv_map) k = p.rows_per_seq >= 3 ? &prefill4_map[npi] : &prefill1_map[npi];
    else k = p.rows_per_seq >= 3 ? &prefill4[npi] : &prefill1[npi];
    grid = dim3(B * p.H * (p.rows_per_seq >= 3 ? ccx_cdiv(p.rows_per_seq, 4) : p.rows_per_seq), 1);
  } else if (p.stream_mode && !p.pos && np_need <= 12) {
    CCX_REQUIRE(ctx, final_out, "dec_attention: the streaming cross attention takes the whole key range (nsplit 1)");
    // (without kv_map the streaming kernel has never looked at row_seq: row r reads sequence r)
    k = (p.kv_map && p.row_seq) ? &streaming_map[npi] : &streaming[npi];
    lds = pad;
    CCX_HIP(ctx, k->optin.ensure(ctx->device, (const void*)k->fn, 128 * 1024));
  } else if (p.out_packed) {
    static DecAttnKernel self_image = {"dec_attention_kernel<true,false,true> (self, image)", dec_attention_kernel<true, false, true>};
    k = &self_image;
  } else if (p.ind) {
    static DecAttnKernel self_ind = {"dec_attention_kernel<true,true> (self, indirect)", dec_attention_kernel<true, true>};
    CCX_REQUIRE(ctx, p.pos && final_out && !p.row_seq && p.ind_ld >= 1, "dec_attention: the cache indirection is taken by the self attention of a decode step only");
    k = &self_ind;
  } else {
    k = &split_kv[p.pos != nullptr][final_out];
    if (!final_out) lds = pad;
    if (lds > 0) CCX_HIP(ctx, k->optin.ensure(ctx->device, (const void*)k->fn, 128 * 1024));
  }
  {
    // self-attention length varies per row and is known on the device only: priced at one key (q in, one K/V row, out), so that
    // the launch shows up in the per-kernel times without claiming traffic it may not have moved
    const double keys = p.pos ? 1.0 : (double)p.T;
    ccx_prof_scope ps(ctx, stream, k->label, 4.0 * B * p.H * keys * 64 * (prefill ? p.rows_per_seq : 1), (double)B * p.H * keys * 64 * 2 * 2);
    hipLaunchKernelGGL(k->fn, grid, dim3(256), lds, stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// ------------------------------------------------------------------------------------------
// Logit filters + greedy selection + per-sequence state machine
// ------------------------------------------------------------------------------------------
// One block (1024 threads) per sequence.  The whole logit row (<= 53248 values) is loaded ONCE
// into registers (13 float4 per thread, all loads issued before any use) together with the
// suppress mask; every reduction then runs out of registers.  The row load, the no-speech softmax and the
// filter (SuppressBlank / SuppressTokens / ApplyTimestampRules, the force-timestamp rule, the log-normaliser)
// are dec_head_row.h's, shared with dec_beam_topk_kernel (dec_beam.hip); what is written here is the prompt
// phase, the draw, the truncation, the per-sequence state machine and the input embedding of the NEXT step
// (token + position), so the step chain needs no separate embed launch.
// Philox4x32-10 (Salmon et al., SC'11): counter-based, so every (seed, sequence, step, vocabulary quad) has its own
// four 32-bit draws regardless of launch geometry.  oracle/whisper_ref.py::philox4x32 is the same function in numpy.
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * ctr.x, p1 = (unsigned long long)0xCD9E8D57u * ctr.z;
    ctr = make_uint4((unsigned)(p1 >> 32) ^ ctr.y ^ key.x, (unsigned)p1, (unsigned)(p0 >> 32) ^ ctr.w ^ key.y, (unsigned)p0);
    key.x += 0x9E3779B9u; key.y += 0xBB67AE85u;
  }
  return ctr;
}
// standard Gumbel noise from a 32-bit draw: u = (x + 0.5) / 2^32 in (0, 1), g = -log(-log(u))
__device__ __forceinline__ float gumbel_from_u32(unsigned x) {
  const float u = ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f);   // 24 bits: exact in fp32, never 0 or 1
  return -logf(-logf(u));
}

#include "dec_head_row.h"
#include "dec_truncate.h"
#include "dec_logprobs.h"
// SAMPLE = false is the greedy kernel (no noise code, no extra registers: the sampling branch costs the 1024-thread
// block its register budget and spills); SAMPLE = true adds the temperature > 0 draw.
// RULES = false is the decode without ApplyTimestampRules (ccx_decode_options.without_timestamps): its own instantiations, so that
// the ruled ones keep their code and their registers.
// TRUNC = true (SAMPLE only) cuts the filtered row by top_k / top_p / min_p before the draw (dec_truncate.h; ccx_decode_sampling_options,
// the three values behind {temperature, seed} in sample_cfg): again its own instantiations, for the same reason.
// LOGP = true (ccx_decode_logprob_options; dec_logprobs.h) stores the log-probability the step adds to sum_logprob and the row's
// top_n (id, log-probability) pairs: once more its own instantiations of all six, so that the six without it keep their code.
template <bool SAMPLE, bool RULES = true, bool TRUNC = false, bool LOGP = false>
__global__ __launch_bounds__(1024) void dec_select_kernel(DecSelectParams p) {
  __shared__ float sh[16];
  __shared__ float sh_v[16];
  __shared__ int sh_i[16];
  __shared__ int sh_next[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.n_vocab;
  const float* lg = p.logits + (long)b * p.ld_logits;
  DecSeqState s = p.state[b];  // every thread reads the same struct ...
  __syncthreads();             // ... before thread 0 may overwrite it below

  auto embed_next = [&](int tok, int pos) {
    // x[b] = tok_emb[tok] + pos_emb[pos]  (TextDecoder.forward input of the next step)
    const float4* te = (const float4*)(p.tok_emb + (long)tok * p.D);
    const float4* pe = (const float4*)(p.pos_emb + (long)pos * p.D);
    float4* xo = (float4*)(p.x + (long)b * p.D);
    for (int i = tid; i < p.D / 4; i += blockDim.x) {
      const float4 a = te[i], c = pe[i];
      xo[i] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
    }
  };

  // ---- prompt phase: feed the next prompt token, nothing is sampled ----
  if (s.pos < s.prompt_len - 1) {
    const int np = s.pos + 1;
    const int tok = p.prompt[(long)b * p.max_prompt + np];
    embed_next(tok, np);
    if (tid == 0) {
      s.pos = np;
      p.cur_tok[b] = tok;
      p.pos[b] = np;
      p.state[b] = s;
    }
    return;
  }
  if (s.done) {  // finished rows keep emitting eot; the model input stays as it is
    if (tid == 0 && s.n_gen < p.sample_len) {
      p.gen[(long)b * p.sample_len + s.n_gen] = p.eot;
      s.n_gen += 1;
      p.state[b] = s;
    }
    return;
  }

  // ---- the shared head (dec_head_row.h): row + mask into registers, no-speech probability, filter ----
  float val[kHeadV4 * 4];
  const unsigned long long sup = head_load_row(tid, lg, p.suppress_mask, V, val);
  const int i_gen = s.n_gen;
  const int tsb = p.timestamp_begin;
  if (i_gen == 0) {
    const float nsp = head_no_speech(tid, lg, p.no_speech, val, sh);
    if (tid == 0) s.no_speech_prob = nsp;
  }
  const HeadFilter f = head_filter<RULES>(tid, p, s, val, sup, sh, sh_v, sh_i);
  // without the rules there is no timestamp side: stated here as constants, so that the tail below folds as it always did
  const float bt = f.bt, bs = RULES ? f.bs : -INFINITY, mx_all = f.mx_all, lnorm = f.lnorm;
  const int it = f.it, is = RULES ? f.is : 0x7fffffff;
  const bool force_ts = RULES && f.force_ts;

  // ---- temperature > 0: Categorical(logits / T) by the Gumbel-max trick (argmax of logits / T + Gumbel noise) ----
  const float temperature = SAMPLE ? __uint_as_float(p.sample_cfg[0]) : 0.f;
  int samp = -1; float samp_logit = 0.f;
  if (SAMPLE && temperature > 0.f) {
    const uint2 key = make_uint2(p.sample_cfg[1], p.sample_cfg[2]);
    const float inv_t = 1.0f / temperature;
    // the row's noise stream: its batch row, or what the caller's table names (rows of a window subset / best_of candidates keep
    // the stream they have in any other launch geometry)
    const unsigned sid = p.stream_id ? (unsigned)p.stream_id[b] : (unsigned)(p.row0 + b);
    float cut = -INFINITY;
    if constexpr (TRUNC) {
      // the row as the draw sees it: a forced-timestamp row has lost its text ids.  lnorm, taken above, stays the normaliser of the
      // untruncated row, so sum_logprob keeps its meaning
      const float m_row = force_ts ? bs : mx_all;
      if (force_ts) {
#pragma unroll
        for (int i = 0; i < kHeadV4 * 4; i++) val[i] = (head_id(tid, i) < tsb) ? -INFINITY : val[i];
      }
      if (m_row > -INFINITY)      // a row with nothing allowed: as without truncation
        cut = dec_trunc::row_cut(val, m_row, temperature, (int)p.sample_cfg[3], __uint_as_float(p.sample_cfg[4]), __uint_as_float(p.sample_cfg[5]),
                                 sh, sh_i, p.kept_out ? p.kept_out + b : nullptr, p.kept_mass_out ? p.kept_mass_out + b : nullptr);
      if (tid == 0 && p.cut_out) p.cut_out[b] = cut;
    }
    float best = -INFINITY, best_logit = -INFINITY; int best_i = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < kHeadV4; i++) {
      const int v0 = tid * 4 + i * 4096;
      const uint4 r = philox4x32_10(make_uint4((unsigned)(v0 >> 2), sid, (unsigned)i_gen, 0u), key);
      const unsigned rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int v = v0 + j;
        float x = (force_ts && v < tsb) ? -INFINITY : val[4 * i + j];
        if constexpr (TRUNC) x = (x < cut) ? -INFINITY : x;
        const float sc = x * inv_t + gumbel_from_u32(rr[j]);      // -inf stays -inf
        if (sc > best) { best = sc; best_i = v; best_logit = x; }
      }
    }
    float ov; int oi;
    block_argmax(tid, best, best_i, ov, oi, sh_v, sh_i);
    samp = oi;
    __syncthreads();
    if (best_i == samp && best == ov) sh[0] = best_logit;         // exactly one thread owns the winner
    __syncthreads();
    samp_logit = sh[0];
  }

  if constexpr (LOGP) {
    // the row's top_n out of the registers the draw is done with: the row as sum_logprob sees it (unscaled, untruncated, no noise),
    // so a forced-timestamp row loses its text ids first where the truncation above has not already taken them
    if (force_ts && !(TRUNC && temperature > 0.f)) {
#pragma unroll
      for (int i = 0; i < kHeadV4 * 4; i++) val[i] = (head_id(tid, i) < tsb) ? -INFINITY : val[i];
    }
    const long at = ((long)b * p.sample_len + i_gen) * kLogprobMaxTop;
    dec_logp::top_rounds(tid, val, p.top_n, mx_all, lnorm, p.top_id + at, p.top_lp + at, sh_v, sh_i);
  }

  if (tid == 0) {
    int next; float logprob;
    if (samp >= 0) {
      next = samp;
      logprob = (samp_logit - mx_all) - lnorm;
    } else if (force_ts) {
      next = is;
      logprob = (bs - mx_all) - lnorm;   // log_softmax over the re-filtered logits (text banned)
    } else {
      if (bt > bs || (bt == bs && it < is)) next = it; else next = is;
      logprob = -lnorm;                 // the winner is mx_all itself
    }
    if (!RULES && (unsigned)next >= (unsigned)V) next = p.eot;   // a call whose list suppresses every id: the row ends
    s.sum_logprob += logprob;
    p.gen[(long)b * p.sample_len + i_gen] = next;
    if constexpr (LOGP) p.tok_logprob[(long)b * p.sample_len + i_gen] = logprob;
    s.n_gen = i_gen + 1;
    s.pen_tok = s.last_tok;
    s.last_tok = next;
    if (next >= tsb) s.last_ts_tok = next;
    int cont = 0;
    if (next == p.eot) {
      s.done = 1;
      s.n_tokens = i_gen;  // tokens before the first eot
      atomicAdd(p.n_done, 1);
    } else if (s.n_gen >= p.sample_len) {
      s.done = 1;
      s.n_tokens = s.n_gen;
      atomicAdd(p.n_done, 1);
    } else {
      s.pos += 1;
      p.cur_tok[b] = next;
      p.pos[b] = s.pos;
      cont = 1;
    }
    p.state[b] = s;
    sh_next[0] = cont ? next : -1;
    sh_next[1] = s.pos;
  }
  __syncthreads();
  if (sh_next[0] >= 0) embed_next(sh_next[0], sh_next[1]);
}

int ccx_launch_dec_embed(ccx_ctx* ctx, const float* tok_emb, const float* pos_emb, const int* cur_tok, const int* pos,
                         float* x, int B, int D, hipStream_t stream) {
  hipLaunchKernelGGL(dec_embed_kernel, dim3(B), dim3(192), 0, stream, tok_emb, pos_emb, cur_tok, pos, x, D);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dec_select(ccx_ctx* ctx, const DecSelectParams& p, int B, hipStream_t stream) {
  ccx_prof_scope ps(ctx, stream, p.trunc ? (p.no_rules ? "dec_select_kernel (truncated, no rules)" : "dec_select_kernel (truncated)") : p.no_rules ? "dec_select_kernel (no rules)" : "dec_select_kernel", 0.0, (double)B * p.n_vocab * 5.0);     // the logit row + its suppress mask
  if (p.tok_logprob) {
    // per-token log-probabilities: the LOGP instantiations of the same six
    if (p.top_n < 0 || p.top_n > kLogprobMaxTop || (p.top_n > 0 && (!p.top_id || !p.top_lp)))
      return ccx_fail(ctx, CCX_ERR_ARG, "dec_select: top_n = %d out of range [0, %d], or top_id / top_lp null", p.top_n, kLogprobMaxTop);
    if (p.trunc && !p.sample) return ccx_fail(ctx, CCX_ERR_ARG, "dec_select: truncation needs the sampling kernel");
    const dim3 g(B), t(1024);
    if (p.trunc) {
      if (p.no_rules) hipLaunchKernelGGL((dec_select_kernel<true, false, true, true>), g, t, 0, stream, p);
      else hipLaunchKernelGGL((dec_select_kernel<true, true, true, true>), g, t, 0, stream, p);
    } else if (p.no_rules) {
      if (p.sample) hipLaunchKernelGGL((dec_select_kernel<true, false, false, true>), g, t, 0, stream, p);
      else hipLaunchKernelGGL((dec_select_kernel<false, false, false, true>), g, t, 0, stream, p);
    } else if (p.sample) hipLaunchKernelGGL((dec_select_kernel<true, true, false, true>), g, t, 0, stream, p);
    else hipLaunchKernelGGL((dec_select_kernel<false, true, false, true>), g, t, 0, stream, p);
  } else if (p.trunc) {
    // truncated sampling: the instantiations with the top_k / top_p / min_p block (a plan sets it only with sampling on)
    if (!p.sample) return ccx_fail(ctx, CCX_ERR_ARG, "dec_select: truncation needs the sampling kernel");
    if (p.no_rules) hipLaunchKernelGGL((dec_select_kernel<true, false, true>), dim3(B), dim3(1024), 0, stream, p);
    else hipLaunchKernelGGL((dec_select_kernel<true, true, true>), dim3(B), dim3(1024), 0, stream, p);
  } else if (p.no_rules) {
    if (p.sample) hipLaunchKernelGGL((dec_select_kernel<true, false>), dim3(B), dim3(1024), 0, stream, p);
    else hipLaunchKernelGGL((dec_select_kernel<false, false>), dim3(B), dim3(1024), 0, stream, p);
  } else if (p.sample) hipLaunchKernelGGL(dec_select_kernel<true>, dim3(B), dim3(1024), 0, stream, p);
  else hipLaunchKernelGGL(dec_select_kernel<false>, dim3(B), dim3(1024), 0, stream, p);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// align.hip -- word alignment on the GPU: what openai-whisper's timing.py::find_alignment computes between the teacher-forced pass and
// the word boundaries [UPSTREAM-RECALL], behind transcribe(word_timestamps=True) of the reference (back/api.py:1435, 1477).
//   align_scores_kernel   softmax over the first n_keys keys of the cross-attention scores of the selected heads (fp32)
//   align_matrix_kernel   standardise over tokens, median-of-7 over frames, mean over heads
//   align_dtw_kernel      anti-diagonal DTW wavefront + backtrace, bit for bit a plain fp32 host loop
// and ccx_align_op, the stand-alone entry point of the three launchers for kernel parity tests (include/ccx.h).  Plain HIP C++, fp32,
// wave64, gfx950.  None of it is on the decode path: an instance that never aligns launches none of these.
#include <vector>
#include "../../include/ccx.h"
#include "align.h"
#include "op_scratch.h"

namespace {

constexpr int kTile = 64;            // frames of one matrix block
constexpr int kCols = kTile + 6;     // ... plus the median's halo of 3 on either side
constexpr int kColPad = 72;          // row pitch of the per-head statistics in LDS

__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
  v = is_max ? wave_reduce_max(v) : wave_reduce_sum(v);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();                   // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < nw; i++) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  return r;
}

// One block per (sequence, selected head): thread j takes keys j, j + 256, ...; a key row is 64 bf16 = eight 16-byte loads.
__global__ __launch_bounds__(256) void align_scores_kernel(AlignScoresParams p) {
  __shared__ float sq[64];
  __shared__ float sc[CCX_ALIGN_MAX_FRAMES];
  __shared__ float red[4];
  const int seq = blockIdx.x, head = p.heads[blockIdx.y], hs = p.hsel[blockIdx.y], tid = threadIdx.x;
  const int n = p.n_keys[seq];
  if (tid < 64) sq[tid] = p.q[((long)seq * p.H + head) * 64 + tid];
  __syncthreads();
  const bf16_t* kb = p.k + ((long)seq * p.H + head) * (long)p.Spad * 64;
  float lmax = -__builtin_inff();
  for (int j = tid; j < n; j += 256) {
    const uint4* kr = (const uint4*)(kb + (long)j * 64);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const uint4 v = kr[c];
      const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        acc = fmaf(sq[c * 8 + 2 * e], __uint_as_float(u[e] << 16), acc);
        acc = fmaf(sq[c * 8 + 2 * e + 1], __uint_as_float(u[e] & 0xffff0000u), acc);
      }
    }
    const float s = acc * 0.125f;
    sc[j] = s;
    lmax = fmaxf(lmax, s);
  }
  const float m = block_reduce(lmax, red, true);
  float lsum = 0.f;
  for (int j = tid; j < n; j += 256) {
    const float e = expf(sc[j] - m);
    sc[j] = e;
    lsum += e;
  }
  const float sum = block_reduce(lsum, red, false);
  float* out = p.P + (((long)seq * p.Hsel + hs) * p.T + p.t) * (long)p.Mmax;
  for (int j = tid; j < p.Mmax; j += 256) out[j] = j < n ? sc[j] / sum : 0.f;
}

// One block per (64-frame tile, sequence).  Phase 1: wave w takes heads w, w + 4, ...: lane = column of the tile (+ halo), mean and
// population std over the token rows in two sequential passes (one summation order).  Phase 2: wave w takes token rows w, w + 4, ...;
// lane = frame; per head the seven standardised neighbours are sorted (odd-even transposition: a true order statistic, ties included).
__global__ __launch_bounds__(256) void align_matrix_kernel(AlignMatrixParams p) {
  extern __shared__ float stats[];       // mean [Hsel][kColPad], then std [Hsel][kColPad]
  const int seq = blockIdx.y, j0 = blockIdx.x * kTile, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int T = p.n_rows[seq], M = p.n_keys[seq];
  if (j0 >= M) return;
  const float* P = p.P + (long)seq * p.Hsel * p.T * (long)p.Mmax;
  float* mean = stats;
  float* sd = stats + p.Hsel * kColPad;
  // frame of column c of the tile: reflect padding (M > 3 makes every reflected index valid); columns no frame of this tile needs
  // are clamped into the row
  auto frame_of = [&](int c) {
    int f = j0 - 3 + c;
    if (f < 0) f = -f;
    if (f >= M) f = 2 * (M - 1) - f;
    return f < 0 ? 0 : (f >= M ? M - 1 : f);
  };
  for (int h = w; h < p.Hsel; h += 4) {
    for (int c = lane; c < kCols; c += 64) {
      const float* col = P + (long)h * p.T * p.Mmax + frame_of(c);
      float s = 0.f;
      for (int t = 0; t < T; t++) s += col[(long)t * p.Mmax];
      const float mu = s / (float)T;
      float v = 0.f;
      for (int t = 0; t < T; t++) {
        const float d = col[(long)t * p.Mmax] - mu;
        v = fmaf(d, d, v);
      }
      mean[h * kColPad + c] = mu;
      sd[h * kColPad + c] = sqrtf(v / (float)T);
    }
  }
  __syncthreads();
  const int j = j0 + lane;
  if (j >= M) return;
  const bool filt = M > 3;
  int fr[7];
#pragma unroll
  for (int d = 0; d < 7; d++) fr[d] = frame_of(lane + d);
  float* A = p.A + (long)seq * p.T * (long)p.Mmax;
  const float n_h = (float)p.Hsel;
  for (int t = w; t < T; t += 4) {
    float acc = 0.f;
    for (int h = 0; h < p.Hsel; h++) {
      const float* row = P + ((long)h * p.T + t) * p.Mmax;
      const float* mu = mean + h * kColPad + lane;
      const float* sg = sd + h * kColPad + lane;
      float med;
      if (filt) {
        float v[7];
#pragma unroll
        for (int d = 0; d < 7; d++) v[d] = (row[fr[d]] - mu[d]) / sg[d];
#pragma unroll
        for (int r = 0; r < 7; r++) {
#pragma unroll
          for (int a = r & 1; a + 1 < 7; a += 2) {
            const float lo = fminf(v[a], v[a + 1]), hi = fmaxf(v[a], v[a + 1]);
            v[a] = lo; v[a + 1] = hi;
          }
        }
        med = v[3];
      } else {
        med = (row[j] - mu[3]) / sg[3];
      }
      acc += med;
    }
    A[(long)t * p.Mmax + j] = acc / n_h;
  }
}

// One block per sequence, thread i - 1 owns text row i (1-based) and walks its columns as the anti-diagonals d = i + j pass.  A cell
// needs cost[i-1][j-1] (c0), cost[i-1][j] (c1) and cost[i][j-1] (c2): c2 is the thread's own last result, c1 comes from the row above
// through a double-buffered LDS line (one barrier per diagonal) and becomes the next cell's c0.  Every cell is ONE fp32 add of two
// determined operands, so the visiting order does not show in the result.  Border row / column of the cost table are +inf
// (cost[0][0] = 0) and are not stored; the backtrace (thread 0) treats them as "left" / "up" as upstream's does.
__global__ __launch_bounds__(512) void align_dtw_kernel(AlignDtwParams p) {
  __shared__ float diag[2][512];
  __shared__ int s_len;
  const int seq = blockIdx.x, tid = threadIdx.x;
  const int M = p.n_keys[seq], N = p.r1[seq] - p.r0;
  const float inf = __builtin_inff();
  const float* A = p.A + (long)seq * p.T * (long)p.Mmax;
  unsigned char* tr = p.trace + (long)seq * p.trace_stride;     // [(N + 1)][(M + 1)]
  int* ti = p.text_idx + (long)seq * p.path_cap;
  int* tj = p.time_idx + (long)seq * p.path_cap;
  int* jf = p.jump_frame + (long)seq * p.T;
  for (int k = tid; k < p.T; k += 512) jf[k] = -1;
  const int i = tid + 1;
  const bool live = i <= N;
  const float* xr = A + (long)(p.r0 + (live ? i - 1 : 0)) * p.Mmax;
  float c2 = inf;                          // cost[i][0]
  float c0 = i == 1 ? 0.f : inf;           // cost[i - 1][0]
  float xn = live ? -xr[0] : 0.f;          // x[i - 1][0], loaded one diagonal ahead
  for (int d = 2; d <= N + M; d++) {
    const int j = d - i;
    if (live && j >= 1 && j <= M) {
      const float x = xn;
      if (j < M) xn = -xr[j];
      const float c1 = i == 1 ? inf : diag[(d - 1) & 1][tid - 1];
      float c; unsigned char t;
      if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
      else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
      else { c = c2; t = 2; }
      const float cost = x + c;
      tr[(long)i * (M + 1) + j] = t;
      diag[d & 1][tid] = cost;
      c2 = cost;
      c0 = c1;
    }
    __syncthreads();
  }
  // backtrace from (N, M), written from the back of the path buffers (the length is known at the end only)
  const int cap = N + M - 1;
  if (tid == 0) {
    int bi = N, bj = M, k = 0;
    while ((bi > 0 || bj > 0) && k < cap) {
      ti[cap - 1 - k] = bi - 1;
      tj[cap - 1 - k] = bj - 1;
      if (bi >= 1) jf[bi - 1] = bj - 1;    // the last visit of a text index is its first path cell
      const int t = bi == 0 ? 2 : (bj == 0 ? 1 : tr[(long)bi * (M + 1) + bj]);
      if (t == 0) { bi--; bj--; }
      else if (t == 1) bi--;
      else bj--;
      k++;
    }
    s_len = k;
    p.path_len[seq] = k;
  }
  __syncthreads();
  const int len = s_len, off = cap - len;
  for (int base = 0; base < len; base += 512) {   // shift the path to the front, chunk by chunk (reads run ahead of the writes)
    const int idx = base + tid;
    int a = 0, b = 0;
    if (idx < len) { a = ti[off + idx]; b = tj[off + idx]; }
    __syncthreads();
    if (idx < len) { ti[idx] = a; tj[idx] = b; }
    __syncthreads();
  }
}

}  // namespace

int ccx_launch_align_scores(ccx_ctx* ctx, const AlignScoresParams& p, int n_seq, hipStream_t stream) {
  CCX_REQUIRE(ctx, n_seq >= 1 && p.n_heads >= 1 && p.Mmax >= 1 && p.Mmax <= CCX_ALIGN_MAX_FRAMES,
              "align_scores: n_seq = %d, n_heads = %d or Mmax = %d out of range", n_seq, p.n_heads, p.Mmax);
  {
    ccx_prof_scope ps(ctx, stream, "align_scores_kernel", 2.0 * n_seq * p.n_heads * 64.0 * p.Mmax, (double)n_seq * p.n_heads * p.Mmax * (128.0 + 4.0));
    hipLaunchKernelGGL(align_scores_kernel, dim3(n_seq, p.n_heads), dim3(256), 0, stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_align_matrix(ccx_ctx* ctx, const AlignMatrixParams& p, int n_seq, hipStream_t stream) {
  CCX_REQUIRE(ctx, n_seq >= 1 && n_seq <= 65535 && p.Hsel >= 1 && p.Hsel <= CCX_ALIGN_MAX_HEADS && p.Mmax >= 1,
              "align_matrix: n_seq = %d, Hsel = %d (at most %d) or Mmax = %d out of range", n_seq, p.Hsel, CCX_ALIGN_MAX_HEADS, p.Mmax);
  {
    ccx_prof_scope ps(ctx, stream, "align_matrix_kernel", 0.0, (double)n_seq * p.Hsel * p.T * p.Mmax * 4.0);
    hipLaunchKernelGGL(align_matrix_kernel, dim3(ccx_cdiv(p.Mmax, kTile), n_seq), dim3(256), (size_t)2 * p.Hsel * kColPad * sizeof(float), stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_align_dtw(ccx_ctx* ctx, const AlignDtwParams& p, int n_seq, hipStream_t stream) {
  CCX_REQUIRE(ctx, n_seq >= 1 && p.T >= 1 && p.T <= CCX_ALIGN_MAX_TOK && p.Mmax >= 1 && p.path_cap >= 1,
              "align_dtw: n_seq = %d, T = %d (at most %d) or Mmax = %d out of range", n_seq, p.T, CCX_ALIGN_MAX_TOK, p.Mmax);
  {
    ccx_prof_scope ps(ctx, stream, "align_dtw_kernel", 0.0, (double)n_seq * p.T * p.Mmax * 5.0);
    hipLaunchKernelGGL(align_dtw_kernel, dim3(n_seq), dim3(512), 0, stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

// ---- the three launchers as a stand-alone operator of the C ABI -------------------------------------------------------------
#define ALIGN_BUF(field, need)                                                                                                      \
  do {                                                                                                                              \
    CCX_REQUIRE(ctx, d->field != nullptr, "ccx_align_op: %s is NULL", #field);                                                      \
    CCX_REQUIRE(ctx, ccx_aligned16(d->field), "ccx_align_op: %s is not 16-byte aligned", #field);                                       \
    CCX_REQUIRE(ctx, d->field##_elems >= (int64_t)(need), "ccx_align_op: %s is accessed up to element %ld, %s_elems=%ld", #field,   \
                (long)(need), #field, (long)d->field##_elems);                                                                      \
  } while (0)
#define ALIGN_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

extern "C" int ccx_align_op(ccx_ctx* ctx, int op, const ccx_align_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_align_op: desc is NULL");
  CCX_REQUIRE(ctx, op >= CCX_ALIGN_SCORES && op <= CCX_ALIGN_DTW, "ccx_align_op: unknown op %d", op);
  const int n_seq = d->n_seq, Hsel = d->Hsel, T = d->T, Mmax = d->Mmax;
  CCX_REQUIRE(ctx, n_seq >= 1 && n_seq <= 4096, "ccx_align_op: n_seq = %d out of range [1, 4096]", n_seq);
  CCX_REQUIRE(ctx, Hsel >= 1 && Hsel <= CCX_ALIGN_MAX_HEADS, "ccx_align_op: Hsel = %d out of range [1, %d]", Hsel, CCX_ALIGN_MAX_HEADS);
  CCX_REQUIRE(ctx, T >= 1 && T <= CCX_ALIGN_MAX_TOK, "ccx_align_op: T = %d out of range [1, %d]", T, CCX_ALIGN_MAX_TOK);
  CCX_REQUIRE(ctx, Mmax >= 1 && Mmax <= CCX_ALIGN_MAX_FRAMES, "ccx_align_op: Mmax = %d out of range [1, %d]", Mmax, CCX_ALIGN_MAX_FRAMES);
  CCX_REQUIRE(ctx, d->n_keys != nullptr, "ccx_align_op: n_keys is NULL");
  int max_keys = 0;
  for (int s = 0; s < n_seq; s++) {
    CCX_REQUIRE(ctx, d->n_keys[s] >= 1 && d->n_keys[s] <= Mmax, "ccx_align_op: n_keys[%d] = %d out of range [1, Mmax = %d]", s, d->n_keys[s], Mmax);
    if (d->n_keys[s] > max_keys) max_keys = d->n_keys[s];
  }
  const int64_t p_need = (int64_t)n_seq * Hsel * T * Mmax, a_need = (int64_t)n_seq * T * Mmax;
  int max_rows = 0;
  if (op == CCX_ALIGN_SCORES) {
    CCX_REQUIRE(ctx, d->H >= 1 && d->H <= 64, "ccx_align_op: H = %d out of range [1, 64]", d->H);
    CCX_REQUIRE(ctx, d->Spad >= 1 && d->Spad <= (1 << 20), "ccx_align_op: Spad = %d out of range [1, 2^20]", d->Spad);
    for (int s = 0; s < n_seq; s++)
      CCX_REQUIRE(ctx, d->n_keys[s] <= d->Spad, "ccx_align_op: n_keys[%d] = %d exceeds Spad = %d", s, d->n_keys[s], d->Spad);
    CCX_REQUIRE(ctx, d->heads != nullptr && d->n_heads >= 1, "ccx_align_op: heads is NULL or n_heads = %d < 1", d->n_heads);
    CCX_REQUIRE(ctx, d->head0 >= 0 && d->n_heads <= Hsel - d->head0, "ccx_align_op: head0 = %d with n_heads = %d leaves the Hsel = %d heads of P", d->head0,
                d->n_heads, Hsel);
    for (int i = 0; i < d->n_heads; i++)
      CCX_REQUIRE(ctx, d->heads[i] >= 0 && d->heads[i] < d->H, "ccx_align_op: heads[%d] = %d out of range [0, H = %d)", i, d->heads[i], d->H);
    CCX_REQUIRE(ctx, d->t >= 0 && d->t < T, "ccx_align_op: t = %d out of range [0, T = %d)", d->t, T);
    ALIGN_BUF(q, (int64_t)n_seq * d->H * 64);
    ALIGN_BUF(k, (int64_t)n_seq * d->H * d->Spad * 64);
    ALIGN_BUF(P, p_need);
  } else {
    CCX_REQUIRE(ctx, d->n_rows != nullptr, "ccx_align_op: n_rows is NULL");
    for (int s = 0; s < n_seq; s++) {
      if (op == CCX_ALIGN_MATRIX)
        CCX_REQUIRE(ctx, d->n_rows[s] >= 2 && d->n_rows[s] <= T, "ccx_align_op: n_rows[%d] = %d out of range [2, T = %d] (a std over one row is 0)", s, d->n_rows[s], T);
      else
        CCX_REQUIRE(ctx, d->r0 >= 0 && d->r0 < d->n_rows[s] && d->n_rows[s] <= T, "ccx_align_op: r0 = %d, n_rows[%d] = %d: need 0 <= r0 < r1 <= T = %d", d->r0, s,
                    d->n_rows[s], T);
      if (d->n_rows[s] > max_rows) max_rows = d->n_rows[s];
    }
    if (op == CCX_ALIGN_MATRIX) {
      ALIGN_BUF(P, p_need);
      ALIGN_BUF(A, a_need);
      CCX_REQUIRE(ctx, d->A != d->P, "ccx_align_op: A aliases P");
    } else {
      ALIGN_BUF(A, a_need);
      ALIGN_BUF(text_idx, (int64_t)n_seq * (T + Mmax));
      ALIGN_BUF(time_idx, (int64_t)n_seq * (T + Mmax));
      ALIGN_BUF(path_len, n_seq);
      ALIGN_BUF(jump_frame, (int64_t)n_seq * T);
    }
  }

  ccx_op_scratch sc;
  int *d_keys = nullptr, *d_rows = nullptr, *d_heads = nullptr, *d_hsel = nullptr;
  ALIGN_HIP(sc.upload(&d_keys, d->n_keys, (size_t)n_seq));
  int rc = CCX_OK;
  if (op == CCX_ALIGN_SCORES) {
    std::vector<int> hsel(d->n_heads);
    for (int i = 0; i < d->n_heads; i++) hsel[i] = d->head0 + i;
    ALIGN_HIP(sc.upload(&d_heads, d->heads, (size_t)d->n_heads));
    ALIGN_HIP(sc.upload(&d_hsel, (const int*)hsel.data(), hsel.size()));
    AlignScoresParams p{(const float*)d->q, (const bf16_t*)d->k, d->H, d->Spad, d_heads, d_hsel, d->n_heads, d_keys, (float*)d->P, Hsel, T, Mmax, d->t};
    rc = ccx_launch_align_scores(ctx, p, n_seq, st);
  } else if (op == CCX_ALIGN_MATRIX) {
    ALIGN_HIP(sc.upload(&d_rows, d->n_rows, (size_t)n_seq));
    AlignMatrixParams p{(const float*)d->P, (float*)d->A, Hsel, T, Mmax, d_rows, d_keys};
    rc = ccx_launch_align_matrix(ctx, p, n_seq, st);
  } else {
    ALIGN_HIP(sc.upload(&d_rows, d->n_rows, (size_t)n_seq));
    unsigned char* trace = nullptr;
    const long stride = (long)(max_rows - d->r0 + 1) * (max_keys + 1);
    ALIGN_HIP(sc.alloc(&trace, (size_t)stride * n_seq));
    AlignDtwParams p{(const float*)d->A, T, Mmax, d->r0, d_rows, d_keys, trace, stride, (int*)d->text_idx, (int*)d->time_idx, T + Mmax,
                     (int*)d->path_len, (int*)d->jump_frame};
    rc = ccx_launch_align_dtw(ctx, p, n_seq, st);
  }
  ALIGN_HIP(hipStreamSynchronize(st));      // the scratch is freed on return
  return rc;
}

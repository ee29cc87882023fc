// dec_probs.hip -- softmax of a logit row over an id range: argmax, the probability of one picked id and (optionally) all
// probabilities of the range.  Two users in whisper.hip:
//  * the no-speech probability of a decode whose SOT sequence has more than one token (multilingual checkpoints: [sot, language,
//    task]) or whose vocabulary is not a multiple of 4: softmax over [0, n_vocab) of the logits AT THE SOT POSITION, pick = <|nospeech|>
//    (openai-whisper decoding.py::DecodingTask._main_loop, `probs_at_sot = logits[:, self.sot_index].float().softmax(dim=-1)`);
//  * language detection: softmax over the contiguous language tokens of the logits of [sot]
//    (decoding.py::detect_language, `mask[list(tokenizer.all_language_tokens)] = False; logits[:, mask] = -np.inf`).
// Also the stand-alone operator ccx_dec_token_probs of the C ABI (include/ccx.h) for kernel parity tests.
#include <math.h>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "decoder.h"
#include "op_scratch.h"

namespace {

#define TP_V4 13   // float4 per thread: 1024 threads x 13 x 4 = 53248 ids

// One block (1024 threads) per row.  The float4 grid starts at `lo` rounded down to 4 (the row base is 16-byte aligned and ld is a
// multiple of 4, so every float4 is aligned and ends at or before ld); no float4 behind the one that holds id hi - 1 is loaded (only the
// 4096-id rounds the range reaches load at all; within them a thread past the end loads the last float4 again), all loads are
// issued before any use, and every element carries its own predicate lo <= id < hi -- values outside the range (NaN,
// the columns [n_vocab, ld)) are replaced by -inf with a select, never by arithmetic, so they cannot leak.  The row is read once;
// every reduction runs out of registers.  fp32 throughout, max-subtracted; -inf inside the range contributes exp2(-inf) = 0.
// A range whose entries are all -inf gives argmax = lo and NaN probabilities, and a +inf inside the range gives NaN probabilities
// too (inf - inf), both as torch.softmax does; a NaN inside the range is the caller's to avoid (the model's logits are finite).
__global__ __launch_bounds__(1024) void dec_token_probs_kernel(DecTokenProbsParams p) {
  __shared__ float sh_v[16];
  __shared__ int sh_i[16];
  __shared__ float sh_s[16];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* lg = p.logits + (long)row * p.ld;
  const int base = p.lo & ~3;

  const int rounds = (p.hi - base + 4095) >> 12;   // 4096-id rounds of the block that hold an id of the range (1 for the language tokens)
  float val[TP_V4 * 4];
#pragma unroll
  for (int i = 0; i < TP_V4; i++) {
    const int v0 = base + tid * 4 + i * 4096;
    // unconditional, at a clamped address (the last float4 that holds an id below hi; hi rounded up to 4 <= ld): straight-line
    // loads that the compiler issues back to back; what a clamped load brings is out of range and dropped by the predicates below
    const int last4 = (p.hi - 1) & ~3;
    float4 f = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (i < rounds) f = *(const float4*)(lg + (v0 < last4 ? v0 : last4));   // block-uniform: rounds the range does not reach load nothing
    val[4 * i] = f.x; val[4 * i + 1] = f.y; val[4 * i + 2] = f.z; val[4 * i + 3] = f.w;
  }
  float mx = -INFINITY;
  int am = 0x7fffffff;
  unsigned long long inb = 0;   // bit i: element i of this thread lies inside [lo, hi) (52 predicates kept as such would not fit the scalar registers)
#pragma unroll
  for (int i = 0; i < TP_V4 * 4; i++) {
    const int v = base + tid * 4 + (i >> 2) * 4096 + (i & 3);
    const bool in = v >= p.lo && v < p.hi;
    const float x = in ? val[i] : -INFINITY;
    val[i] = x;
    inb |= (unsigned long long)(in ? 1 : 0) << i;
    // ids ascend within a thread: a strictly larger value wins, and so does the first in-range id while nothing is held
    const bool better = in && (x > mx || am == 0x7fffffff);
    mx = better ? x : mx; am = better ? v : am;
  }
  // block argmax, lowest id on equal values (dec_select_kernel and torch.argmax on the CPU use the same rule)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(am, o, 64);
    if (ov > mx || (ov == mx && oi < am)) { mx = ov; am = oi; }
  }
  if ((tid & 63) == 0) { sh_v[tid >> 6] = mx; sh_i[tid >> 6] = am; }
  __syncthreads();
  float bmx = sh_v[0]; int bam = sh_i[0];
  for (int w = 1; w < 16; w++)
    if (sh_v[w] > bmx || (sh_v[w] == bmx && sh_i[w] < bam)) { bmx = sh_v[w]; bam = sh_i[w]; }

  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < TP_V4 * 4; i++) sum += __builtin_amdgcn_exp2f((val[i] - bmx) * 1.4426950408889634f);
  sum = wave_reduce_sum(sum);
  if ((tid & 63) == 0) sh_s[tid >> 6] = sum;
  __syncthreads();
  float tot = 0.f;
  for (int w = 0; w < 16; w++) tot += sh_s[w];

  if (tid == 0) {
    p.argmax[row] = bam;
    // pick lies inside [lo, hi); the same operations as probs[pick - lo] below, so that the two outputs carry the same bits
    p.pick_prob[row] = __builtin_amdgcn_exp2f((lg[p.pick] - bmx) * 1.4426950408889634f) / tot;
  }
  if (p.probs) {
    float* pr = p.probs + (long)row * (p.hi - p.lo);
#pragma unroll
    for (int i = 0; i < TP_V4 * 4; i++) {
      const int v = base + tid * 4 + (i >> 2) * 4096 + (i & 3);
      if ((inb >> i) & 1) pr[v - p.lo] = __builtin_amdgcn_exp2f((val[i] - bmx) * 1.4426950408889634f) / tot;
    }
  }
}

}  // namespace

int ccx_launch_dec_token_probs(ccx_ctx* ctx, const DecTokenProbsParams& p, int rows, hipStream_t stream) {
  CCX_REQUIRE(ctx, p.logits && p.argmax && p.pick_prob && rows >= 1, "dec_token_probs: null argument or no rows");
  CCX_REQUIRE(ctx, p.lo >= 0 && p.lo < p.hi && p.hi <= p.ld && p.ld % 4 == 0 && p.hi - (p.lo & ~3) <= TP_V4 * 4096,
              "dec_token_probs: range [%d, %d) does not fit ld = %ld or the %d ids a block holds", p.lo, p.hi, p.ld, TP_V4 * 4096);
  CCX_REQUIRE(ctx, p.pick >= p.lo && p.pick < p.hi, "dec_token_probs: pick = %d outside [%d, %d)", p.pick, p.lo, p.hi);
  CCX_REQUIRE(ctx, ((uintptr_t)p.logits & 15) == 0, "dec_token_probs: logits must be 16-byte aligned");
  const double n = (double)rows * (p.hi - p.lo);
  ccx_prof_scope ps(ctx, stream, "dec_token_probs_kernel", 0.0, n * 4.0 + (p.probs ? n * 4.0 : 0.0));
  hipLaunchKernelGGL(dec_token_probs_kernel, dim3(rows), dim3(1024), 0, stream, p);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

extern "C" int ccx_dec_token_probs(ccx_ctx* ctx, const ccx_dec_token_probs_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_token_probs: desc is NULL");
  const int V = d->n_vocab, rows = d->rows;
  CCX_REQUIRE(ctx, rows >= 1 && rows <= 65536, "ccx_dec_token_probs: rows = %d out of range [1, 65536]", rows);
  CCX_REQUIRE(ctx, V >= 1 && V <= TP_V4 * 4096, "ccx_dec_token_probs: n_vocab = %d out of range [1, %d]", V, TP_V4 * 4096);
  CCX_REQUIRE(ctx, d->ld >= V && d->ld % 4 == 0 && d->ld <= (1 << 24), "ccx_dec_token_probs: ld = %ld must be >= n_vocab = %d and a multiple of 4", (long)d->ld, V);
  CCX_REQUIRE(ctx, d->lo >= 0 && d->lo < d->hi, "ccx_dec_token_probs: lo = %d, hi = %d is not a range", d->lo, d->hi);
  CCX_REQUIRE(ctx, d->hi <= V, "ccx_dec_token_probs: hi = %d behind n_vocab = %d", d->hi, V);
  CCX_REQUIRE(ctx, d->pick >= d->lo && d->pick < d->hi, "ccx_dec_token_probs: pick = %d outside [lo = %d, hi = %d)", d->pick, d->lo, d->hi);
  CCX_REQUIRE(ctx, d->logits && ccx_aligned16(d->logits), "ccx_dec_token_probs: logits null or not 16-byte aligned");
  // the last float4 a row loads ends at hi rounded up to 4
  const int64_t need = (int64_t)(rows - 1) * d->ld + ((d->hi + 3) & ~3);
  CCX_REQUIRE(ctx, need <= d->logits_elems, "ccx_dec_token_probs: logits are read up to element %ld, logits_elems = %ld", (long)need, (long)d->logits_elems);
  CCX_REQUIRE(ctx, d->argmax && d->pick_prob, "ccx_dec_token_probs: argmax or pick_prob is NULL");
  if (d->probs) {
    CCX_REQUIRE(ctx, ((uintptr_t)d->probs & 3) == 0, "ccx_dec_token_probs: probs is not 4-byte aligned");
    const int64_t pn = (int64_t)rows * (d->hi - d->lo);
    CCX_REQUIRE(ctx, pn <= d->probs_elems, "ccx_dec_token_probs: probs is written up to element %ld, probs_elems = %ld", (long)pn, (long)d->probs_elems);
  }
#define DO_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
  ccx_op_scratch sc;
  int* d_arg = nullptr; float* d_pp = nullptr;
  DO_HIP(sc.alloc(&d_arg, (size_t)rows));
  DO_HIP(sc.alloc(&d_pp, (size_t)rows));
  DecTokenProbsParams p;
  memset(&p, 0, sizeof(p));
  p.logits = (const float*)d->logits; p.ld = (long)d->ld; p.lo = d->lo; p.hi = d->hi; p.pick = d->pick;
  p.argmax = d_arg; p.pick_prob = d_pp; p.probs = (float*)d->probs;
  CCX_TRY(ccx_launch_dec_token_probs(ctx, p, rows, stream));
  DO_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
  DO_HIP(hipMemcpy(d->argmax, d_arg, (size_t)rows * 4, hipMemcpyDeviceToHost));
  DO_HIP(hipMemcpy(d->pick_prob, d_pp, (size_t)rows * 4, hipMemcpyDeviceToHost));
#undef DO_HIP
  return CCX_OK;
}

// dec_probs.hip -- softmax of a logit row over an id range: argmax, the probability of one picked id and (optionally) all
// probabilities of the range.  Two users in whisper.hip:
//  * the no-speech probability of a decode whose SOT sequence has more than one token (multilingual checkpoints: [sot, language,
//    task]) or whose vocabulary is not a multiple of 4: softmax over [0, n_vocab) of the logits AT THE SOT POSITION, pick = <|nospeech|>
//    (openai-whisper decoding.py::DecodingTask._main_loop, `probs_at_sot = logits[:, self.sot_index].float().softmax(dim=-1)`);
//  * language detection: softmax over the contiguous language tokens of the logits of [sot]
//    (decoding.py::detect_language, `mask[list(tokenizer.all_language_tokens)] = False; logits[:, mask] = -np.inf`).
// dec_pick_probs_kernel shares the row pass and gives the probability of one picked id PER ROW over [0, hi): the word probabilities
// of the alignment pass (ccx_whisper_align_probs; openai-whisper timing.py::find_alignment, `token_probs = logits[len(sot_sequence):,
// :eot].softmax(dim=-1)`, `text_token_probs = token_probs[np.arange(len(text_tokens)), text_tokens]`).
// Also the stand-alone operators ccx_dec_token_probs and ccx_dec_pick_probs of the C ABI (include/ccx.h) for kernel parity tests.
#include <math.h>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "dec_head_row.h"   // kHeadV4, kHeadMaxVocab: a block holds what the head kernels' blocks hold
#include "op_scratch.h"

namespace {


// The row pass both kernels share: one block (1024 threads) reads the ids [lo, hi) of the row `lg` once and leaves them in `val`
// (everything outside the range as -inf), bit i of `inb` = element i of this thread lies inside the range, and returns the block's
// maximum `bmx`, its argmax `bam` (lowest id on equal values) and the sum `tot` of exp(x - bmx) over the range.
// The float4 grid starts at `lo` rounded down to 4 (the row base is 16-byte aligned and ld is a
// multiple of 4, so every float4 is aligned and ends at or before ld); no float4 behind the one that holds id hi - 1 is loaded (only the
// 4096-id rounds the range reaches load at all; within them a thread past the end loads the last float4 again), all loads are
// issued before any use, and every element carries its own predicate lo <= id < hi -- values outside the range (NaN,
// the columns [n_vocab, ld)) are replaced by -inf with a select, never by arithmetic, so they cannot leak.  The row is read once;
// every reduction runs out of registers.  fp32 throughout, max-subtracted; -inf inside the range contributes exp2(-inf) = 0.
// A range whose entries are all -inf gives argmax = lo and NaN probabilities, and a +inf inside the range gives NaN probabilities
// too (inf - inf), both as torch.softmax does; a NaN inside the range is the caller's to avoid (the model's logits are finite).
__device__ __forceinline__ void tp_row_pass(const float* lg, int lo, int hi, float (&val)[kHeadV4 * 4], unsigned long long& inb_out,
                                            float& bmx_out, int& bam_out, float& tot_out) {
  __shared__ float sh_v[16];
  __shared__ int sh_i[16];
  __shared__ float sh_s[16];
  const int tid = threadIdx.x;
  const int base = lo & ~3;

  const int rounds = (hi - base + 4095) >> 12;   // 4096-id rounds of the block that hold an id of the range (1 for the language tokens)
#pragma unroll
  for (int i = 0; i < kHeadV4; i++) {
    const int v0 = base + tid * 4 + i * 4096;
    // unconditional, at a clamped address (the last float4 that holds an id below hi; hi rounded up to 4 <= ld): straight-line
    // loads that the compiler issues back to back; what a clamped load brings is out of range and dropped by the predicates below
    const int last4 = (hi - 1) & ~3;
    float4 f = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (i < rounds) f = *(const float4*)(lg + (v0 < last4 ? v0 : last4));   // block-uniform: rounds the range does not reach load nothing
    val[4 * i] = f.x; val[4 * i + 1] = f.y; val[4 * i + 2] = f.z; val[4 * i + 3] = f.w;
  }
  float mx = -INFINITY;
  int am = 0x7fffffff;
  unsigned long long inb = 0;   // bit i: element i of this thread lies inside [lo, hi) (52 predicates kept as such would not fit the scalar registers)
#pragma unroll
  for (int i = 0; i < kHeadV4 * 4; i++) {
    const int v = base + tid * 4 + (i >> 2) * 4096 + (i & 3);
    const bool in = v >= lo && v < hi;
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
  for (int i = 0; i < kHeadV4 * 4; i++) sum += __builtin_amdgcn_exp2f((val[i] - bmx) * 1.4426950408889634f);
  sum = wave_reduce_sum(sum);
  if ((tid & 63) == 0) sh_s[tid >> 6] = sum;
  __syncthreads();
  float tot = 0.f;
  for (int w = 0; w < 16; w++) tot += sh_s[w];
  inb_out = inb; bmx_out = bmx; bam_out = bam; tot_out = tot;
}

__global__ __launch_bounds__(1024) void dec_token_probs_kernel(DecTokenProbsParams p) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* lg = p.logits + (long)row * p.ld;
  const int base = p.lo & ~3;
  float val[kHeadV4 * 4];
  unsigned long long inb;
  float bmx, tot;
  int bam;
  tp_row_pass(lg, p.lo, p.hi, val, inb, bmx, bam, tot);

  if (tid == 0) {
    p.argmax[row] = bam;
    // pick lies inside [lo, hi); the same operations as probs[pick - lo] below, so that the two outputs carry the same bits
    p.pick_prob[row] = __builtin_amdgcn_exp2f((lg[p.pick] - bmx) * 1.4426950408889634f) / tot;
  }
  if (p.probs) {
    float* pr = p.probs + (long)row * (p.hi - p.lo);
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) {
      const int v = base + tid * 4 + (i >> 2) * 4096 + (i & 3);
      if ((inb >> i) & 1) pr[v - p.lo] = __builtin_amdgcn_exp2f((val[i] - bmx) * 1.4426950408889634f) / tot;
    }
  }
}

// The probability of ONE picked id per row over the ids [0, hi): out[row * out_stride] = exp(x[pick] - max) / sum_{j < hi} exp(x[j] - max)
// with pick = picks[row * pick_stride].  A row whose pick is negative is skipped: its block returns before it loads anything and
// writes nothing.  The host checks that every other pick lies below hi (a pick behind hi is skipped too, never read).  The strides
// let a caller walk column t of [rows][T] tables without uploading anything per step (ccx_whisper_align_probs: upstream's
// timing.py::find_alignment, `logits[len(sot_sequence):, :eot].softmax(-1)[arange(len(text_tokens)), text_tokens]`).
__global__ __launch_bounds__(1024) void dec_pick_probs_kernel(DecPickProbsParams p) {
  const int row = blockIdx.x;
  const int pick = p.picks[(long)row * p.pick_stride];
  if (pick < 0 || pick >= p.hi) return;      // block-uniform
  const float* lg = p.logits + (long)row * p.ld;
  float val[kHeadV4 * 4];
  unsigned long long inb;
  float bmx, tot;
  int bam;
  tp_row_pass(lg, 0, p.hi, val, inb, bmx, bam, tot);
  // the same operations as dec_token_probs_kernel's pick_prob
  if (threadIdx.x == 0) p.out[(long)row * p.out_stride] = __builtin_amdgcn_exp2f((lg[pick] - bmx) * 1.4426950408889634f) / tot;
}

}  // namespace

int ccx_launch_dec_token_probs(ccx_ctx* ctx, const DecTokenProbsParams& p, int rows, hipStream_t stream) {
  CCX_REQUIRE(ctx, p.logits && p.argmax && p.pick_prob && rows >= 1, "dec_token_probs: null argument or no rows");
  CCX_REQUIRE(ctx, p.lo >= 0 && p.lo < p.hi && p.hi <= p.ld && p.ld % 4 == 0 && p.hi - (p.lo & ~3) <= kHeadMaxVocab,
              "dec_token_probs: range [%d, %d) does not fit ld = %ld or the %d ids a block holds", p.lo, p.hi, p.ld, kHeadMaxVocab);
  CCX_REQUIRE(ctx, p.pick >= p.lo && p.pick < p.hi, "dec_token_probs: pick = %d outside [%d, %d)", p.pick, p.lo, p.hi);
  CCX_REQUIRE(ctx, ((uintptr_t)p.logits & 15) == 0, "dec_token_probs: logits must be 16-byte aligned");
  const double n = (double)rows * (p.hi - p.lo);
  ccx_prof_scope ps(ctx, stream, "dec_token_probs_kernel", 0.0, n * 4.0 + (p.probs ? n * 4.0 : 0.0));
  hipLaunchKernelGGL(dec_token_probs_kernel, dim3(rows), dim3(1024), 0, stream, p);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_launch_dec_pick_probs(ccx_ctx* ctx, const DecPickProbsParams& p, int rows, hipStream_t stream) {
  CCX_REQUIRE(ctx, p.logits && p.picks && p.out && rows >= 1, "dec_pick_probs: null argument or no rows");
  CCX_REQUIRE(ctx, p.hi >= 1 && p.hi <= p.ld && p.ld % 4 == 0 && p.hi <= kHeadMaxVocab,
              "dec_pick_probs: range [0, %d) does not fit ld = %ld or the %d ids a block holds", p.hi, p.ld, kHeadMaxVocab);
  CCX_REQUIRE(ctx, p.pick_stride >= 1 && p.out_stride >= 1, "dec_pick_probs: pick_stride = %ld, out_stride = %ld must be >= 1", p.pick_stride, p.out_stride);
  CCX_REQUIRE(ctx, ((uintptr_t)p.logits & 15) == 0, "dec_pick_probs: logits must be 16-byte aligned");
  ccx_prof_scope ps(ctx, stream, "dec_pick_probs_kernel", 0.0, (double)rows * p.hi * 4.0 + rows * 8.0);
  hipLaunchKernelGGL(dec_pick_probs_kernel, dim3(rows), dim3(1024), 0, stream, p);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

extern "C" int ccx_dec_token_probs(ccx_ctx* ctx, const ccx_dec_token_probs_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_token_probs: desc is NULL");
  const int V = d->n_vocab, rows = d->rows;
  CCX_REQUIRE(ctx, rows >= 1 && rows <= 65536, "ccx_dec_token_probs: rows = %d out of range [1, 65536]", rows);
  CCX_REQUIRE(ctx, V >= 1 && V <= kHeadMaxVocab, "ccx_dec_token_probs: n_vocab = %d out of range [1, %d]", V, kHeadMaxVocab);
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

extern "C" int ccx_dec_pick_probs(ccx_ctx* ctx, const ccx_dec_pick_probs_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_pick_probs: desc is NULL");
  const int rows = d->rows, hi = d->hi;
  CCX_REQUIRE(ctx, rows >= 1 && rows <= 65536, "ccx_dec_pick_probs: rows = %d out of range [1, 65536]", rows);
  CCX_REQUIRE(ctx, hi >= 1 && hi <= kHeadMaxVocab, "ccx_dec_pick_probs: hi = %d out of range [1, %d]", hi, kHeadMaxVocab);
  CCX_REQUIRE(ctx, d->ld >= hi && d->ld % 4 == 0 && d->ld <= (1 << 24), "ccx_dec_pick_probs: ld = %ld must be >= hi = %d and a multiple of 4", (long)d->ld, hi);
  CCX_REQUIRE(ctx, d->logits && ccx_aligned16(d->logits), "ccx_dec_pick_probs: logits null or not 16-byte aligned");
  // the last float4 a row loads ends at hi rounded up to 4
  const int64_t need = (int64_t)(rows - 1) * d->ld + ((hi + 3) & ~3);
  CCX_REQUIRE(ctx, need <= d->logits_elems, "ccx_dec_pick_probs: logits are read up to element %ld, logits_elems = %ld", (long)need, (long)d->logits_elems);
  CCX_REQUIRE(ctx, d->pick_stride >= 1 && d->pick_stride <= (1 << 24), "ccx_dec_pick_probs: pick_stride = %ld out of range [1, %d]", (long)d->pick_stride, 1 << 24);
  CCX_REQUIRE(ctx, d->out_stride >= 1 && d->out_stride <= (1 << 24), "ccx_dec_pick_probs: out_stride = %ld out of range [1, %d]", (long)d->out_stride, 1 << 24);
  CCX_REQUIRE(ctx, d->picks && ((uintptr_t)d->picks & 3) == 0, "ccx_dec_pick_probs: picks null or not 4-byte aligned");
  CCX_REQUIRE(ctx, d->out && ((uintptr_t)d->out & 3) == 0, "ccx_dec_pick_probs: out null or not 4-byte aligned");
  const int64_t pn = (int64_t)(rows - 1) * d->pick_stride + 1, on = (int64_t)(rows - 1) * d->out_stride + 1;
  CCX_REQUIRE(ctx, pn <= d->picks_elems, "ccx_dec_pick_probs: picks are read up to element %ld, picks_elems = %ld", (long)pn, (long)d->picks_elems);
  CCX_REQUIRE(ctx, on <= d->out_elems, "ccx_dec_pick_probs: out is written up to element %ld, out_elems = %ld", (long)on, (long)d->out_elems);
#define DO_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
  // the picks live on the device: one copy to the host, so that no id the kernel would read behind hi is ever launched
  std::vector<int32_t> host((size_t)pn);
  DO_HIP(hipStreamSynchronize(stream));
  DO_HIP(hipMemcpy(host.data(), d->picks, (size_t)pn * 4, hipMemcpyDeviceToHost));
  for (int r = 0; r < rows; r++) {
    const int32_t pk = host[(size_t)r * d->pick_stride];
    CCX_REQUIRE(ctx, pk == -1 || (pk >= 0 && pk < hi), "ccx_dec_pick_probs: picks of row %d = %d is neither -1 nor inside [0, hi = %d)", r, pk, hi);
  }
  DecPickProbsParams p;
  memset(&p, 0, sizeof(p));
  p.logits = (const float*)d->logits; p.ld = (long)d->ld; p.hi = hi;
  p.picks = (const int*)d->picks; p.pick_stride = (long)d->pick_stride; p.out = (float*)d->out; p.out_stride = (long)d->out_stride;
  CCX_TRY(ccx_launch_dec_pick_probs(ctx, p, rows, stream));
  DO_HIP(hipStreamSynchronize(stream));
#undef DO_HIP
  return CCX_OK;
}

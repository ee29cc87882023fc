// dec_history.hip -- the two decoding rules that read a row's own sampled history: repetition_penalty and no_repeat_ngram_size
// (the form of Hugging Face's RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor, which CTranslate2 / faster-whisper
// expose under the same names; the rule is ours and is restated in tests/history_rules_reference.py; parity unpinned).  They cannot
// live in the static suppress masks, so dec_head (whisper.hip) launches dec_history_kernel between the logits GEMM and the select /
// beam top-k kernel of a decode that sets them (ccx_whisper_set_history_options): it edits the fp32 logit row in place, and everything
// behind it -- SuppressBlank, SuppressTokens, ApplyTimestampRules, the sampler, sum_logprob -- sees the edited row.  A default decode
// never launches it.  Also the stand-alone operator ccx_dec_history_step of the C ABI (include/ccx.h) for kernel parity tests.
//
// For one row in the sampling phase, H = gen[0 : m], m = n_gen (what THIS decode sampled: no prompt, SOT sequence or prefix), E =
// text_end (rules.eot; ids >= E -- eot, the specials, the timestamps -- are never edited, so the timestamp rules and closed pairs
// <|t|><|t|> keep working):
//   1. penalty p != 1: for every distinct v in H with v < E: x = logits[v]; logits[v] = x > 0 ? x / p : x * p (each id once)
//   2. n-gram ban n >= 1, m >= n: for every j in [n - 1, m) with H[j - n + 1 : j] == H[m - n + 1 : m] and H[j] < E: logits[H[j]] = -inf
//      (the matched context may hold ids >= E; n = 1 bans every text id sampled so far)
//   1 before 2: an id both penalised and banned ends at -inf.  Rows that are done or still in the prompt phase are not touched.
#include <math.h>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "decoder.h"
#include "dec_head_row.h"
#include "op_scratch.h"

namespace {

// One block per row.  The history is staged in LDS (kDecHistoryMax ids: sample_len is at most n_text_ctx - 1 = 447 in every Whisper).
// Penalty: the thread that holds H[t] acts only if no t' < t holds the same id -- no atomics, no id edited twice.  The barrier behind
// it makes the edits visible block-wide before a ban may hit the same id.  Ban: the thread that holds H[j] compares the n - 1 ids
// before it with the history's last n - 1; duplicate -inf stores are harmless.  Every store lands on an id in [0, text_end) of the
// block's own row: an id outside that range (never sampled by the select kernel) is skipped, not trusted.
__global__ __launch_bounds__(256) void dec_history_kernel(DecHistoryParams p) {
  __shared__ int sh_h[kDecHistoryMax];
  const int row = blockIdx.x, tid = threadIdx.x;
  const DecSeqState* st = p.state + row;
  if (st->done || st->pos < st->prompt_len - 1) return;            // block-uniform
  const int n_gen = st->n_gen;
  const int m = n_gen < p.sample_len ? n_gen : p.sample_len;
  if (m <= 0) return;                                              // block-uniform
  const int* gen = p.gen + (long)row * p.sample_len;
  for (int t = tid; t < m; t += 256) sh_h[t] = gen[t];
  __syncthreads();
  float* lg = p.logits + (long)row * p.ld;
  const int E = p.text_end, n = p.ngram;
  if (p.penalty != 1.f) {
    for (int t = tid; t < m; t += 256) {
      const int v = sh_h[t];
      if (v < 0 || v >= E) continue;
      bool first = true;
      for (int u = 0; u < t; u++) first = first && sh_h[u] != v;
      if (first) {
        const float x = lg[v];
        lg[v] = x > 0.f ? x / p.penalty : x * p.penalty;
      }
    }
  }
  __syncthreads();
  if (n >= 1 && m >= n) {
    for (int j = n - 1 + tid; j < m; j += 256) {
      const int v = sh_h[j];
      if (v < 0 || v >= E) continue;
      bool eq = true;
      for (int k = 1; k < n; k++) eq = eq && sh_h[j - k] == sh_h[m - k];
      if (eq) lg[v] = -INFINITY;
    }
  }
}

}  // namespace

int ccx_launch_dec_history(ccx_ctx* ctx, const DecHistoryParams& p, int rows, hipStream_t stream) {
  CCX_REQUIRE(ctx, p.logits && p.state && p.gen && rows >= 1, "dec_history: null argument or no rows");
  CCX_REQUIRE(ctx, p.sample_len >= 1 && p.sample_len <= kDecHistoryMax, "dec_history: sample_len = %d out of range [1, %d]", p.sample_len, kDecHistoryMax);
  CCX_REQUIRE(ctx, p.text_end >= 0 && p.text_end <= p.ld, "dec_history: text_end = %d out of range [0, ld = %ld]", p.text_end, p.ld);
  CCX_REQUIRE(ctx, p.penalty > 0.f && p.penalty <= 3.4028234e38f && p.ngram >= 0, "dec_history: penalty %g must be finite and > 0, ngram %d >= 0", (double)p.penalty, p.ngram);
  // a row reads its state and history and reads / writes one logit per distinct id
  ccx_prof_scope ps(ctx, stream, "dec_history_kernel", 0.0, (double)rows * (sizeof(DecSeqState) + p.sample_len * 12.0));
  hipLaunchKernelGGL(dec_history_kernel, dim3(rows), dim3(256), 0, stream, p);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

extern "C" void ccx_decode_history_options_default(ccx_decode_history_options* o) {
  if (o) *o = ccx_decode_history_options{1.0f, 0};
}

extern "C" int ccx_dec_history_step(ccx_ctx* ctx, const ccx_dec_history_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_history_step: desc is NULL");
  const int V = d->n_vocab, R = d->rows, SL = d->sample_len;
  CCX_REQUIRE(ctx, R >= 1 && R <= 65536, "ccx_dec_history_step: rows = %d out of range [1, 65536]", R);
  CCX_REQUIRE(ctx, V >= 1 && V <= kHeadMaxVocab, "ccx_dec_history_step: n_vocab = %d out of range [1, 53248]", V);
  CCX_REQUIRE(ctx, d->ld >= V && d->ld <= (1 << 24), "ccx_dec_history_step: ld = %ld must be >= n_vocab = %d", (long)d->ld, V);
  CCX_REQUIRE(ctx, d->logits && ((uintptr_t)d->logits & 3) == 0, "ccx_dec_history_step: logits null or not 4-byte aligned");
  CCX_REQUIRE(ctx, (int64_t)(R - 1) * d->ld + V <= d->logits_elems, "ccx_dec_history_step: logits are written up to element %ld, logits_elems = %ld",
              (long)((int64_t)(R - 1) * d->ld + V), (long)d->logits_elems);
  CCX_REQUIRE(ctx, d->state && d->hist, "ccx_dec_history_step: state or hist is NULL");
  CCX_REQUIRE(ctx, SL >= 1 && SL <= kDecHistoryMax, "ccx_dec_history_step: sample_len = %d out of range [1, %d]", SL, kDecHistoryMax);
  CCX_REQUIRE(ctx, d->text_end >= 0 && d->text_end <= V, "ccx_dec_history_step: text_end = %d out of range [0, n_vocab = %d]", d->text_end, V);
  const float pen = d->repetition_penalty;
  CCX_REQUIRE(ctx, pen > 0.f && pen <= 3.4028234e38f, "ccx_dec_history_step: repetition_penalty = %g must be finite and > 0", (double)pen);
  CCX_REQUIRE(ctx, d->no_repeat_ngram_size >= 0, "ccx_dec_history_step: no_repeat_ngram_size = %d is negative", d->no_repeat_ngram_size);
  for (int r = 0; r < R; r++) {
    const ccx_dec_seq_state& s = d->state[r];
    CCX_REQUIRE(ctx, s.n_gen >= 0 && s.n_gen <= SL, "ccx_dec_history_step: state[%d].n_gen = %d out of range [0, sample_len = %d]", r, s.n_gen, SL);
    CCX_REQUIRE(ctx, s.done == 0 || s.done == 1, "ccx_dec_history_step: state[%d].done = %d must be 0 or 1", r, s.done);
    if (s.done || s.pos < s.prompt_len - 1) continue;       // not touched: its history is never read
    for (int t = 0; t < s.n_gen; t++) {
      const int v = d->hist[(size_t)r * SL + t];
      CCX_REQUIRE(ctx, v >= 0 && v < V, "ccx_dec_history_step: hist[%d][%d] = %d out of range [0, n_vocab = %d)", r, t, v, V);
    }
  }
#define DO_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
  ccx_op_scratch sc;
  DecSeqState* d_state = nullptr; int* d_hist = nullptr;
  DO_HIP(sc.upload(&d_state, (const DecSeqState*)d->state, (size_t)R));
  DO_HIP(sc.upload(&d_hist, d->hist, (size_t)R * SL));
  DecHistoryParams p;
  memset(&p, 0, sizeof(p));
  p.logits = (float*)d->logits; p.ld = (long)d->ld; p.state = d_state; p.gen = d_hist; p.sample_len = SL;
  p.text_end = d->text_end; p.penalty = pen; p.ngram = d->no_repeat_ngram_size;
  CCX_TRY(ccx_launch_dec_history(ctx, p, R, stream));
  DO_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
#undef DO_HIP
  return CCX_OK;
}

// dec_bias.hip -- vocabulary control per call: sequence_bias, and through it bad_words_ids and hotwords (the form of Hugging Face's
// SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor; the rule is ours and is restated in tests/bias_reference.py; parity
// unpinned).  The bias on the last id of a phrase depends on what the row has just sampled, so it cannot live in the static suppress
// masks: dec_head (whisper.hip) launches dec_bias_kernel between the logits GEMM and dec_history_kernel / the select / beam top-k
// kernel of a decode that has a table set (ccx_whisper_set_bias_options).  It edits the fp32 logit row in place, and everything behind
// it -- the history rules, SuppressBlank, SuppressTokens, ApplyTimestampRules, the sampler, sum_logprob -- sees the edited row.  A
// decode without a table never launches it.  Also the host-side table compile and the stand-alone operator ccx_dec_bias_step of the
// C ABI (include/ccx.h) for kernel parity tests.
//
// A table is an ordered list of entries (ids[0 .. L), bias), 1 <= L <= 32, target ids[L - 1] < E = text_end (rules.eot; ids >= E are
// never edited), bias finite or -inf.  For one row in the sampling phase, H = gen[0 : m], m = n_gen (what THIS decode sampled: no
// prompt, SOT sequence or prefix):
//   b1[v] = fp32 sum, in table order, of the length-1 entries with target v
//   S[v]  = fp32 sum, in table order, of the entries with L >= 2, target v, L - 1 <= m and H[m - L + 1 : m] == ids[0 : L - 1]
//   logits[v] = (logits[v] + b1[v]) + S[v]; a term that does not exist is skipped (not added as zero); each term lands once per id
// Rows that are done or still in the prompt phase are not touched.  With length-1 entries the row of the first sampled step (m = 0)
// is edited too, and the select kernel's no_speech_prob, read there, is the softmax of the edited row.
#include <math.h>
#include <string.h>
#include <algorithm>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "decoder.h"
#include "dec_head_row.h"
#include "op_scratch.h"

static_assert(kBiasMaxEntries == CCX_BIAS_MAX_ENTRIES && kBiasMaxIds == CCX_BIAS_MAX_IDS && kBiasMaxLen == CCX_BIAS_MAX_LEN,
              "decoder.h's table capacities are the header's");

namespace {

// One block of 256 threads per row; the early exits are block-uniform and come before any barrier.  The last min(m, 31) ids of the
// history -- the longest context -- are staged in LDS.  Phase 1: the distinct (v, b1[v]) pairs, strided over the threads (targets are
// unique: no race).  A barrier makes those edits visible block-wide.  Phase 2: the entries of two and more ids are keyed by their LAST
// context id; the row binary-searches the sorted distinct keys for H[m - 1] and visits that key's groups only (a group: one (key,
// target) pair, its entries in table order), one thread per group: it sums the matching entries in order and does one read-modify-write
// -- no atomics, so the order of the sum and its bits are fixed, and a row never walks the whole table.  Every store lands on an id in
// [0, text_end) of the block's own row; counts and offsets read from the table are clamped to its capacity, not trusted.
__global__ __launch_bounds__(256) void dec_bias_kernel(DecBiasParams p) {
  __shared__ int sh_h[kBiasMaxLen];
  const int row = blockIdx.x, tid = threadIdx.x;
  const DecSeqState* st = p.state + row;
  if (st->done || st->pos < st->prompt_len - 1) return;            // block-uniform
  const int* tab = p.tab;
  const int n1 = min(max(tab[kBiasHdr + 0], 0), kBiasMaxEntries), n_keys = min(max(tab[kBiasHdr + 1], 0), kBiasMaxEntries);
  const int n_gen = st->n_gen;
  const int m = n_gen < p.sample_len ? n_gen : p.sample_len;
  if (n1 == 0 && (n_keys == 0 || m <= 0)) return;                  // block-uniform
  const int k = m < kBiasMaxLen - 1 ? (m > 0 ? m : 0) : kBiasMaxLen - 1;
  if (tid < k) sh_h[tid] = p.gen[(long)row * p.sample_len + (m - k + tid)];
  __syncthreads();
  float* lg = p.logits + (long)row * p.ld;
  const int E = p.text_end;
  for (int i = tid; i < n1; i += 256) {
    const int v = tab[kBiasL1Tgt + i];
    if (v >= 0 && v < E) lg[v] = lg[v] + __int_as_float(tab[kBiasL1Bias + i]);
  }
  __syncthreads();
  if (k == 0 || n_keys == 0) return;
  const int last = sh_h[k - 1];
  int lo = 0, hi = n_keys;                                          // the first key >= last
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[kBiasKey + mid] < last) lo = mid + 1; else hi = mid;
  }
  if (lo >= n_keys || tab[kBiasKey + lo] != last) return;
  const int g0 = max(tab[kBiasKeyOff + lo], 0), g1 = min(tab[kBiasKeyOff + lo + 1], kBiasMaxEntries);
  for (int g = g0 + tid; g < g1; g += 256) {
    const int v = tab[kBiasGrpTgt + g];
    const int e0 = max(tab[kBiasGrpOff + g], 0), e1 = min(tab[kBiasGrpOff + g + 1], kBiasMaxEntries);
    float s = 0.f;
    bool any = false;
    for (int e = e0; e < e1; e++) {
      const int c = tab[kBiasEntLen + e], co = tab[kBiasEntCtx + e];  // the context: c = L - 1 ids at pool offset co
      if (c < 1 || c > k || co < 0 || co + c > kBiasMaxIds) continue;
      bool eq = true;
      for (int j = 0; j < c; j++) eq = eq && tab[kBiasCtx + co + j] == sh_h[k - c + j];
      if (eq) {
        const float b = __int_as_float(tab[kBiasEntBias + e]);
        s = any ? s + b : b;
        any = true;
      }
    }
    if (any && v >= 0 && v < E) lg[v] = lg[v] + s;
  }
}

}  // namespace

int ccx_launch_dec_bias(ccx_ctx* ctx, const DecBiasParams& p, int rows, hipStream_t stream) {
  CCX_REQUIRE(ctx, p.logits && p.state && p.gen && p.tab && rows >= 1, "dec_bias: null argument or no rows");
  CCX_REQUIRE(ctx, p.sample_len >= 1, "dec_bias: sample_len = %d must be >= 1", p.sample_len);
  CCX_REQUIRE(ctx, p.text_end >= 0 && p.text_end <= p.ld, "dec_bias: text_end = %d out of range [0, ld = %ld]", p.text_end, p.ld);
  // a row reads its state, its history's tail, the length-1 list and one key's groups; it reads / writes one logit per term
  ccx_prof_scope ps(ctx, stream, "dec_bias_kernel", 0.0, (double)rows * (sizeof(DecSeqState) + kBiasMaxLen * 4.0));
  hipLaunchKernelGGL(dec_bias_kernel, dim3(rows), dim3(256), 0, stream, p);
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

int ccx_compile_bias_table(ccx_ctx* ctx, const char* who, const ccx_decode_bias_options* o, int V, int E, std::vector<int>& tab,
                           bool* has_len1) {
  tab.assign((size_t)kBiasTabInts, 0);
  if (has_len1) *has_len1 = false;
  if (!o || o->n_entries == 0) return CCX_OK;
  const int n = o->n_entries;
  CCX_REQUIRE(ctx, n >= 0 && n <= kBiasMaxEntries, "%s: opts.n_entries = %d out of range [0, %d]", who, n, kBiasMaxEntries);
  CCX_REQUIRE(ctx, o->offsets && o->ids && o->bias, "%s: opts.offsets, opts.ids or opts.bias is NULL", who);
  const int* off = o->offsets;
  CCX_REQUIRE(ctx, off[0] == 0, "%s: opts.offsets[0] = %d must be 0", who, off[0]);
  for (int e = 0; e < n; e++) {
    CCX_REQUIRE(ctx, off[e + 1] >= off[e], "%s: opts.offsets[%d] = %d does not ascend (offsets[%d] = %d)", who, e + 1, off[e + 1], e, off[e]);
    const int L = off[e + 1] - off[e];
    CCX_REQUIRE(ctx, L >= 1 && L <= kBiasMaxLen, "%s: opts.offsets: entry %d has %d ids, out of range [1, %d]", who, e, L, kBiasMaxLen);
    CCX_REQUIRE(ctx, off[e + 1] <= kBiasMaxIds, "%s: opts.offsets[%d] = %d: more than %d ids in total", who, e + 1, off[e + 1], kBiasMaxIds);
  }
  for (int e = 0; e < n; e++) {
    for (int j = off[e]; j < off[e + 1]; j++)
      CCX_REQUIRE(ctx, o->ids[j] >= 0 && o->ids[j] < V, "%s: opts.ids[%d] = %d (entry %d) out of range [0, n_vocab = %d)", who, j, o->ids[j], e, V);
    const int t = off[e + 1] - 1;
    CCX_REQUIRE(ctx, o->ids[t] < E, "%s: opts.ids[%d] = %d: the target of entry %d must be < eot = %d", who, t, o->ids[t], e, E);
    CCX_REQUIRE(ctx, o->bias[e] <= 3.4028234e38f, "%s: opts.bias[%d] = %g must be finite or -inf", who, e, (double)o->bias[e]);
  }
  auto len = [&](int e) { return off[e + 1] - off[e]; };
  auto tgt = [&](int e) { return o->ids[off[e + 1] - 1]; };
  auto key = [&](int e) { return o->ids[off[e + 1] - 2]; };
  auto bits = [](float f) { int i; memcpy(&i, &f, 4); return i; };
  std::vector<int> one, multi;
  for (int e = 0; e < n; e++) (len(e) == 1 ? one : multi).push_back(e);
  // length-1 entries: stable by target, every target's biases summed in the caller's order
  std::stable_sort(one.begin(), one.end(), [&](int a, int b) { return tgt(a) < tgt(b); });
  int n1 = 0;
  for (size_t i = 0; i < one.size();) {
    const int v = tgt(one[i]);
    float s = o->bias[one[i]];
    size_t j = i + 1;
    for (; j < one.size() && tgt(one[j]) == v; j++) s = s + o->bias[one[j]];
    CCX_REQUIRE(ctx, s <= 3.4028234e38f, "%s: opts.bias: the length-1 entries of target %d sum to %g, neither finite nor -inf", who, v, (double)s);
    tab[kBiasL1Tgt + n1] = v; tab[kBiasL1Bias + n1] = bits(s);
    n1++; i = j;
  }
  // longer entries: stable by (last context id, target); a group is one such pair, its entries in the caller's order
  std::stable_sort(multi.begin(), multi.end(), [&](int a, int b) { return key(a) != key(b) ? key(a) < key(b) : tgt(a) < tgt(b); });
  int n_keys = 0, n_groups = 0, pool = 0;
  for (size_t i = 0; i < multi.size(); i++) {
    const int e = multi[i];
    const bool new_key = i == 0 || key(e) != key(multi[i - 1]);
    if (new_key) { tab[kBiasKey + n_keys] = key(e); tab[kBiasKeyOff + n_keys] = n_groups; n_keys++; }
    if (new_key || tgt(e) != tgt(multi[i - 1])) { tab[kBiasGrpTgt + n_groups] = tgt(e); tab[kBiasGrpOff + n_groups] = (int)i; n_groups++; }
    const int c = len(e) - 1;
    tab[kBiasEntLen + i] = c; tab[kBiasEntCtx + i] = pool; tab[kBiasEntBias + i] = bits(o->bias[e]);
    for (int j = 0; j < c; j++) tab[kBiasCtx + pool + j] = o->ids[off[e] + j];
    pool += c;
  }
  tab[kBiasKeyOff + n_keys] = n_groups;
  tab[kBiasGrpOff + n_groups] = (int)multi.size();
  tab[kBiasHdr + 0] = n1; tab[kBiasHdr + 1] = n_keys; tab[kBiasHdr + 2] = n_groups; tab[kBiasHdr + 3] = (int)multi.size();
  if (has_len1) *has_len1 = n1 > 0;
  return CCX_OK;
}

extern "C" void ccx_decode_bias_options_default(ccx_decode_bias_options* o) {
  if (o) *o = ccx_decode_bias_options{0, nullptr, nullptr, nullptr};
}

extern "C" int ccx_dec_bias_step(ccx_ctx* ctx, const ccx_dec_bias_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_dec_bias_step: desc is NULL");
  const int V = d->n_vocab, R = d->rows, SL = d->sample_len;
  CCX_REQUIRE(ctx, R >= 1 && R <= 65536, "ccx_dec_bias_step: rows = %d out of range [1, 65536]", R);
  CCX_REQUIRE(ctx, V >= 1 && V <= kHeadMaxVocab, "ccx_dec_bias_step: n_vocab = %d out of range [1, 53248]", V);
  CCX_REQUIRE(ctx, d->ld >= V && d->ld <= (1 << 24), "ccx_dec_bias_step: ld = %ld must be >= n_vocab = %d", (long)d->ld, V);
  CCX_REQUIRE(ctx, d->logits && ((uintptr_t)d->logits & 3) == 0, "ccx_dec_bias_step: logits null or not 4-byte aligned");
  CCX_REQUIRE(ctx, (int64_t)(R - 1) * d->ld + V <= d->logits_elems, "ccx_dec_bias_step: logits are written up to element %ld, logits_elems = %ld",
              (long)((int64_t)(R - 1) * d->ld + V), (long)d->logits_elems);
  CCX_REQUIRE(ctx, d->state && d->hist, "ccx_dec_bias_step: state or hist is NULL");
  CCX_REQUIRE(ctx, SL >= 1 && SL <= kDecHistoryMax, "ccx_dec_bias_step: sample_len = %d out of range [1, %d]", SL, kDecHistoryMax);
  CCX_REQUIRE(ctx, d->text_end >= 0 && d->text_end <= V, "ccx_dec_bias_step: text_end = %d out of range [0, n_vocab = %d]", d->text_end, V);
  std::vector<int> tab;
  CCX_TRY(ccx_compile_bias_table(ctx, "ccx_dec_bias_step", &d->table, V, d->text_end, tab, nullptr));
  for (int r = 0; r < R; r++) {
    const ccx_dec_seq_state& s = d->state[r];
    CCX_REQUIRE(ctx, s.n_gen >= 0 && s.n_gen <= SL, "ccx_dec_bias_step: state[%d].n_gen = %d out of range [0, sample_len = %d]", r, s.n_gen, SL);
    CCX_REQUIRE(ctx, s.done == 0 || s.done == 1, "ccx_dec_bias_step: state[%d].done = %d must be 0 or 1", r, s.done);
    if (s.done || s.pos < s.prompt_len - 1) continue;       // not touched: its history is never read
    for (int t = 0; t < s.n_gen; t++) {
      const int v = d->hist[(size_t)r * SL + t];
      CCX_REQUIRE(ctx, v >= 0 && v < V, "ccx_dec_bias_step: hist[%d][%d] = %d out of range [0, n_vocab = %d)", r, t, v, V);
    }
  }
#define DO_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
  ccx_op_scratch sc;
  DecSeqState* d_state = nullptr; int *d_hist = nullptr, *d_tab = nullptr;
  DO_HIP(sc.upload(&d_state, (const DecSeqState*)d->state, (size_t)R));
  DO_HIP(sc.upload(&d_hist, d->hist, (size_t)R * SL));
  DO_HIP(sc.upload(&d_tab, (const int*)tab.data(), tab.size()));
  DecBiasParams p;
  memset(&p, 0, sizeof(p));
  p.logits = (float*)d->logits; p.ld = (long)d->ld; p.state = d_state; p.gen = d_hist; p.sample_len = SL;
  p.text_end = d->text_end; p.tab = d_tab;
  CCX_TRY(ccx_launch_dec_bias(ctx, p, R, stream));
  DO_HIP(hipStreamSynchronize(stream));      // the scratch is freed on return
#undef DO_HIP
  return CCX_OK;
}

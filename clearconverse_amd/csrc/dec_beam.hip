// dec_beam.hip -- the beam-search head of a decode step (openai-whisper decoding.py::BeamSearchDecoder.update [UPSTREAM-RECALL], restated
// in tests/beam_reference.py).  Rows come in windows of `beam` consecutive rows; a step is two launches behind the logits GEMM:
//
//  * dec_beam_topk_kernel, one block per row, the select kernel's (dec_select_kernel, decoder.hip) front half with another tail: the
//    row load, the no-speech softmax and the filter -- suppress mask, timestamp rules, force-timestamp rule, log-normaliser
//    ((x - max) - log(sum)) -- are the functions of dec_head_row.h that the select kernel calls too, so a rule is changed there, once,
//    for both (tests/test_dec_head_agreement_gpu.py holds the two kernels to the same bits).  What is written here is the window
//    prologue and beam + 1 masked block arg-max rounds out of the filtered registers: the row's best (id, log-probability) pairs.
//  * dec_beam_update_kernel, one block per window: ranks the window's beam x (beam + 1) candidates by cumulative score, walks them
//    (eot candidates finish, the others become the next live rows until `beam` are taken), and rewrites the window IN PLACE -- read
//    everything, barrier, write: per-row state, token history, the rows of the self-attention cache indirection, the next step's
//    embedding, the finished tables.  A captured step graph replays with fixed arguments, so nothing alternates between steps.
//
// Tie rule: equal cumulative scores go to the lower source row, then to the lower id (the select kernel's arg-max order).
#include "dec_head_row.h"

namespace {

// RULES = false: the decode without ApplyTimestampRules (ccx_decode_options.without_timestamps), an instantiation of its own as in
// the select kernel (head_filter<false>).
template <bool RULES>
__global__ __launch_bounds__(1024) void dec_beam_topk_kernel(DecBeamParams bp) {
  __shared__ float sh[16];
  __shared__ float sh_v[16];
  __shared__ int sh_i[16];
  const DecSelectParams& p = bp.sel;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = p.n_vocab;
  const int K = bp.beam + 1;
  const float* lg = p.logits + (long)b * p.ld_logits;
  const DecSeqState s = p.state[b];
  if (s.done) return;                        // a complete window is frozen: its candidate rows keep what they hold
  const int i_gen = s.n_gen;
  int* cid = bp.cand_id + (long)b * K;
  float* clp = bp.cand_lp + (long)b * K;
  int* tr_id = bp.tr_cand_id ? bp.tr_cand_id + ((long)i_gen * bp.tr_rows + b) * K : nullptr;
  float* tr_lp = bp.tr_cand_id ? bp.tr_cand_lp + ((long)i_gen * bp.tr_rows + b) * K : nullptr;
  // first sampled step: all rows of a window hold the same prefix (upstream's dict keyed by sequence collapses them), row 0 proposes
  if (i_gen == 0 && (b % bp.beam) != 0) {
    if (tid < K) {
      cid[tid] = -1; clp[tid] = -INFINITY;
      if (tr_id) { tr_id[tid] = -1; tr_lp[tid] = -INFINITY; }
    }
    return;
  }

  float val[kHeadV4 * 4];
  const unsigned long long sup = head_load_row(tid, lg, p.suppress_mask, V, val);
  // the no-speech probability of the first sampled step: the update kernel hands it to every row of the window
  if (i_gen == 0) {
    const float nsp = head_no_speech(tid, lg, p.no_speech, val, sh);
    if (tid == 0) p.state[b].no_speech_prob = nsp;
  }
  const HeadFilter f = head_filter<RULES>(tid, p, s, val, sup, sh, sh_v, sh_i);
  const float mx_all = f.mx_all, lnorm = f.lnorm;
  if (f.force_ts) {                          // the summed timestamp mass beats the best text token: timestamps only
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) val[i] = (head_id(tid, i) < p.timestamp_begin) ? -INFINITY : val[i];
  }
  // ---- the row's top beam + 1: masked block arg-max rounds out of the registers ----
#pragma unroll 1
  for (int k = 0; k < K; k++) {
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) {
      const int v = head_id(tid, i);
      const bool up = val[i] > bv;            // ids ascend with i: the lowest id of equal values stays
      bv = up ? val[i] : bv; bi = up ? v : bi;
    }
    float ov; int oi;
    block_argmax(tid, bv, bi, ov, oi, sh_v, sh_i);
    if (tid == 0) {
      const bool some = ov > -INFINITY;
      const int id = some ? oi : -1;
      const float lp = some ? (ov - mx_all) - lnorm : -INFINITY;
      cid[k] = id; clp[k] = lp;
      if (tr_id) { tr_id[k] = id; tr_lp[k] = lp; }
    }
#pragma unroll
    for (int i = 0; i < kHeadV4 * 4; i++) val[i] = (head_id(tid, i) == oi) ? -INFINITY : val[i];
  }
}

constexpr int kBeamCands = kBeamMax * (kBeamMax + 1);

__global__ __launch_bounds__(256) void dec_beam_update_kernel(DecBeamParams bp) {
  extern __shared__ __attribute__((aligned(16))) int dyn[];
  __shared__ DecSeqState st[kBeamMax];
  __shared__ float sc[kBeamCands];
  __shared__ int cid_s[kBeamCands], order[kBeamCands], fin_list[kBeamCands], fin_slot[kBeamCands];
  __shared__ int surv[kBeamMax], sh_nf, sh_stop, sh_skip;
  const DecSelectParams& p = bp.sel;
  const int beam = bp.beam, K = beam + 1, N = beam * K;
  const int g = blockIdx.x, r0 = g * beam, tid = threadIdx.x, nthr = blockDim.x;
  const int SL = p.sample_len;
  int* hist_s = dyn;                                         // [beam][SL]
  unsigned short* ind_s = (unsigned short*)(dyn + beam * SL);  // [beam][ind_ld]

  if (p.state[r0].done) {                    // complete (or out of budget): the window stays exactly as it is
    if (bp.step_tok && tid < beam) { bp.step_tok[r0 + tid] = -1; bp.step_parent[r0 + tid] = -1; }
    return;
  }
  if (tid < beam) st[tid] = p.state[r0 + tid];
  __syncthreads();
  const int n_gen = st[0].n_gen, pos_old = st[0].pos;        // one prompt per window: its rows step together
  if (tid < N) {
    const int j = tid / K;
    const int id = bp.cand_id[(long)(r0 + j) * K + (tid - j * K)];
    const float lp = bp.cand_lp[(long)(r0 + j) * K + (tid - j * K)];
    cid_s[tid] = id;
    sc[tid] = id >= 0 ? st[j].sum_logprob + lp : -INFINITY;
  }
  for (int e = tid; e < beam * n_gen; e += nthr) {
    const int j = e / n_gen, i = e - j * n_gen;
    hist_s[j * SL + i] = p.gen[(long)(r0 + j) * SL + i];
  }
  for (int e = tid; e < beam * (pos_old + 1); e += nthr) {
    const int j = e / (pos_old + 1), t = e - j * (pos_old + 1);
    ind_s[j * bp.ind_ld + t] = bp.ind[(long)(r0 + j) * bp.ind_ld + t];
  }
  __syncthreads();
  // rank by counting: candidate u stands before t if it is valid and scores higher, or equally with the lower index (= the lower
  // source row, then the earlier arg-max round = the lower id of equal log-probabilities)
  if (tid < N) {
    const bool vt = cid_s[tid] >= 0;
    const float s_t = sc[tid];
    int rank = 0;
    for (int u = 0; u < N; u++) {
      const bool vu = cid_s[u] >= 0;
      const bool before = vu ? (!vt || sc[u] > s_t || (sc[u] == s_t && u < tid)) : (!vt && u < tid);
      rank += before ? 1 : 0;
    }
    order[rank] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    int live = 0, nf = 0;
    for (int c = 0; c < N; c++) {
      const int t = order[c];
      if (cid_s[t] < 0) break;
      if (cid_s[t] == p.eot) fin_list[nf++] = t;
      else { surv[live++] = t; if (live == beam) break; }
    }
    const int skip = live == 0;              // no live continuation at all (nothing but eot is allowed): the window ends here
    for (; live < beam; live++) surv[live] = -1;   // fewer continuations than rows: dead copies of the best one, score -inf
    int cnt = bp.fin_count[g];
    for (int k = 0; k < nf; k++) fin_slot[k] = cnt < bp.max_cand ? cnt++ : -1;
    bp.fin_count[g] = cnt;
    const int stop = skip || cnt >= bp.max_cand || n_gen + 1 >= SL;
    if (stop) atomicAdd(p.n_done, beam);
    sh_nf = nf; sh_stop = stop; sh_skip = skip;
  }
  __syncthreads();
  const int nf = sh_nf, stop = sh_stop, skip = sh_skip;
  // ---- finished hypotheses: the parent's history (the eot itself is not stored) ----
  for (int k = 0; k < nf; k++) {
    if (fin_slot[k] < 0) continue;
    const int t = fin_list[k], j = t / K;
    const long slot = (long)g * bp.max_cand + fin_slot[k];
    for (int i = tid; i < n_gen; i += nthr) bp.fin_tok[slot * SL + i] = hist_s[j * SL + i];
    if (tid == 0) { bp.fin_score[slot] = sc[t]; bp.fin_n[slot] = n_gen; }
  }
  if (skip) {
    if (tid < beam) {
      p.state[r0 + tid].done = 1;
      p.state[r0 + tid].n_tokens = n_gen;
      if (bp.step_tok) { bp.step_tok[r0 + tid] = -1; bp.step_parent[r0 + tid] = -1; }
    }
    return;
  }
  // ---- the next live rows, each from its parent ----
  for (int jj = 0; jj < beam; jj++) {
    const bool dead = surv[jj] < 0;
    const int t = dead ? surv[0] : surv[jj];
    const int pj = t / K, tok = cid_s[t], r = r0 + jj;
    for (int i = tid; i < n_gen; i += nthr) p.gen[(long)r * SL + i] = hist_s[pj * SL + i];
    if (!stop) {
      for (int i = tid; i <= pos_old; i += nthr) bp.ind[(long)r * bp.ind_ld + i] = ind_s[pj * bp.ind_ld + i];
      const float4* te = (const float4*)(p.tok_emb + (long)tok * p.D);
      const float4* pe = (const float4*)(p.pos_emb + (long)(pos_old + 1) * p.D);
      float4* xo = (float4*)(p.x + (long)r * p.D);
      for (int i = tid; i < p.D / 4; i += nthr) {
        const float4 a = te[i], c = pe[i];
        xo[i] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
      }
    }
    if (tid == 0) {
      DecSeqState ns = st[pj];
      const float score = dead ? -INFINITY : sc[t];
      ns.sum_logprob = score;
      p.gen[(long)r * SL + n_gen] = tok;
      ns.n_gen = n_gen + 1;
      ns.pen_tok = ns.last_tok;
      ns.last_tok = tok;
      if (tok >= p.timestamp_begin) ns.last_ts_tok = tok;
      if (stop) {
        ns.done = 1;
        ns.n_tokens = ns.n_gen;
      } else {
        ns.pos = pos_old + 1;
        p.cur_tok[r] = tok;
        p.pos[r] = pos_old + 1;
        bp.ind[(long)r * bp.ind_ld + pos_old + 1] = (unsigned short)(bp.row0 + r);
      }
      p.state[r] = ns;
      if (bp.step_tok) { bp.step_tok[r] = tok; bp.step_parent[r] = r0 + pj; }
      if (bp.tr_tok) {
        const long at = (long)n_gen * bp.tr_rows + r;
        bp.tr_tok[at] = tok; bp.tr_parent[at] = r0 + pj; bp.tr_score[at] = score;
      }
    }
  }
}

}  // namespace

int ccx_launch_dec_beam(ccx_ctx* ctx, const DecBeamParams& p, int n_windows, hipStream_t stream) {
  CCX_REQUIRE(ctx, p.beam >= 1 && p.beam <= kBeamMax && p.max_cand >= 1 && p.max_cand <= kBeamCandMax && n_windows >= 1,
              "dec_beam: beam = %d, max_candidates = %d or windows = %d out of range", p.beam, p.max_cand, n_windows);
  const size_t lds = (size_t)p.beam * p.sel.sample_len * 4 + ccx_align((size_t)p.beam * p.ind_ld * 2, 16);
  CCX_REQUIRE(ctx, lds <= 48 * 1024, "dec_beam: %d rows x (sample_len %d, %d cache positions) need %zu bytes of LDS (at most 49152)", p.beam,
              p.sel.sample_len, p.ind_ld, lds);
  const int rows = n_windows * p.beam;
  {
    ccx_prof_scope ps(ctx, stream, p.sel.no_rules ? "dec_beam_topk_kernel (no rules)" : "dec_beam_topk_kernel", 0.0, (double)rows * p.sel.n_vocab * 5.0);
    if (p.sel.no_rules) hipLaunchKernelGGL(dec_beam_topk_kernel<false>, dim3(rows), dim3(1024), 0, stream, p);
    else hipLaunchKernelGGL(dec_beam_topk_kernel<true>, dim3(rows), dim3(1024), 0, stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  {
    ccx_prof_scope ps(ctx, stream, "dec_beam_update_kernel", 0.0, (double)rows * (p.sel.D * 12.0 + p.sel.sample_len * 8.0 + p.ind_ld * 4.0));
    hipLaunchKernelGGL(dec_beam_update_kernel, dim3(n_windows), dim3(256), lds, stream, p);
  }
  CCX_CHECK_LAUNCH(ctx);
  return CCX_OK;
}

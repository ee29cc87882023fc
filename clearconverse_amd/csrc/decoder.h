// decoder.h -- parameter blocks and launchers for the decoder step kernels (decoder.hip).
#pragma once
#include <cstring>
#include <vector>
#include "../../include/ccx.h"
#include "ccx_common.h"

enum { ACT_LN = 0, ACT_BF16 = 1, ACT_COMBINE = 2 };
// DEPI_RESOLVE: the residual add done by the PRODUCER (no split-K slabs): x[m][n] += acc + bias in place (fp32), a bf16 copy of the new
// row centred by a per-row shift and, per 16-column tile of every row, its (sum, sum of squares) -- the statistics with which the
// cross-attention query of the X-stream path applies its LayerNorm algebraically (dec_xq_lnfree_kernel, cross_x.hip)
enum { DEPI_BF16_GELU = 1, DEPI_PARTIAL = 2, DEPI_F32 = 3, DEPI_SELF_QKV = 4, DEPI_RESOLVE = 5 };

struct DecLinearParams {
  int M, N, K;
  const bf16_t* W; long ldw;      // [N][K]
  const float* bias;              // [N] or null
  // activation sources
  const float* x;                 // ACT_LN: [M][K] f32 residual stream (before the pending partials)
  const float* pend; int pend_n; long pend_stride;  // pending split-K partials [pend_n][M][K] folded into x
  float* x_out;                   // ACT_LN: if non-null, block (0,*,0) writes x + sum(pend) here (must differ from x)
  const float* ln_g; const float* ln_b; float eps;
  float* ln_mean_out;             // ACT_LN: if non-null, block (0,*,0) writes every row's centring shift here [M] (centre_shift)
  const bf16_t* act; long lda;    // ACT_BF16: [M][K]
  const float* part_o; const float* part_ml; int nsplit;  // ACT_COMBINE: [M][H][nsplit][64], [M][H][nsplit][2]
  // DEPI_RESOLVE: xres [M][N] f32 (read and written in place), xb [M][N] bf16, st_out [M][N / 16].  xb and st_out hold the row
  // CENTRED by shift[m] + shift_c (shift null: uncentred): bf16 rounding of an uncentred row costs ~ulp(|mean|) per element, which the
  // LayerNorm the query applies afterwards divides by the row's std (uncentred, |mean| / std >= 40 took the teacher-forced logits of
  // the mini model from rel-L2 5.0e-3 to 1.26e-2: tests/test_whisper_stress_gpu.py)
  float* xres; bf16_t* xb; float2* st_out; const float* shift; float shift_c;
  // outputs (DEPI_PARTIAL: out[z][m][n] with stride pend_stride between the grid.z slices)
  void* out; long ldo;
  // DEPI_SELF_QKV: q -> out (f32 [M][K]), k/v -> caches [sequence][H][cache_T][64] at pos[m]; the sequence of row m is
  // row_seq[m] (prompt prefill: several rows per sequence) or m itself when row_seq is null
  bf16_t* cache_k; bf16_t* cache_v; int cache_T; const int* pos; const int* row_seq;
  // ACT_BF16 only.  act_packed: `act` is the fragment image of the rows instead (dec_frag_off: ceil(M / 16) x K / 32 tiles of 1 KB, so a
  // wave load is 1 KB contiguous and not 16 rows x 64 B; lda is not read).  DEPI_BF16_GELU, out_packed: `out` is written as that
  // image of [M][N] (N a multiple of 32; ldo is not read); DEPI_RESOLVE, out_packed: `xb` is.  The values a lane holds, and so the
  // results, are the same either way.
  int act_packed, out_packed;
};
int ccx_launch_dec_linear(ccx_ctx* ctx, int act, int epi, const DecLinearParams& p, hipStream_t stream);
// number of grid.z K-slices ccx_launch_dec_linear will use (= number of partial slabs written)
int ccx_dec_linear_ksplit(int K, int epi);
// The launcher's rule on K: every one of a block's 4 waves must own a k-step of the block's grid.z slice.  A slice of L k-steps
// (per_z = ceil(K / 32 / ksplit) of them, the last slice what is left) gives a wave per_w = ceil(L / 4); the last wave starts at
// 3 per_w, so the rule is 3 per_w < L -- it fails for L = 1, 2, 3, 5, 6 and 9 (and for an empty slice).  Returns the first slice
// that breaks it and its length in *len, or -1.
static inline int ccx_dec_linear_starved_slice(int K, int ksplit, int* len) {
  const int ksteps = K / 32, per_z = (ksteps + ksplit - 1) / ksplit;
  for (int z = 0; z < ksplit; z++) {
    const int L = ksteps - z * per_z < per_z ? ksteps - z * per_z : per_z;
    if (L <= 0 || 3 * ((L + 3) / 4) >= L) { *len = L; return z; }
  }
  return -1;
}
// out = bf16 LayerNorm(x + sum pend); if x_out != null also writes the resolved x there (must not alias x); if mean_out != null
// also every row's centring shift from its LayerNorm statistics (the same bits the ACT_LN prologue of dec_linear computes)
int ccx_launch_dec_resolve_ln(ccx_ctx* ctx, const float* x, const float* pend, int pend_n, long pend_stride, const float* g,
                              const float* b, bf16_t* out, float* x_out, int M, int K, float eps, hipStream_t stream,
                              float* mean_out = nullptr, int out_packed = 0);

// The fragment image of a bf16 activation matrix [M][K] (K a multiple of 32), the layout pack_mfma_rows gives the weights: tile
// (m / 16, k / 32) holds the 64 lanes' 16-byte MFMA operands back to back, lane l = row m0 + (l & 15), columns k0 + 8 (l >> 4) .. + 7.
// Element offset of (m, k); 8 consecutive k from a multiple of 8 on stay together.  The image takes ceil(M / 16) * 16 * K elements.
__host__ __device__ __forceinline__ long dec_frag_off(int m, int k, int ksteps) {
  return (((long)(m >> 4) * ksteps + (k >> 5)) * 64 + (((k >> 3) & 3) * 16 + (m & 15))) * 8 + (k & 7);
}
// CCX_DEC_PACKED_ACT (default 1; read per decode): the > 16-row chain hands its LayerNorm rows and its GELU rows from kernel to kernel
// as fragment images; 0: row-major, as the <= 16-row chain and every other reader of these buffers keep them
int ccx_dec_packed_act_switch();
// CCX_DEC_PACKED_MID (default 1; read per decode): the same for the rest of that chain's bf16 rows -- dattn (self attention -> out
// projection, value projection -> cross-attention out projection) and xb (out projection -> LayerNorm-free query)
int ccx_dec_packed_mid_switch();
// The rule both switches share: lanes of more than 16 rows in whole 16-row tiles (a lane's image then ends where the next lane's
// begins); every other launch keeps row-major rows.
static inline int ccx_dec_rows_as_image(int on, int rows) { return (on && rows > 16 && rows % 16 == 0) ? 1 : 0; }

struct DecAttnParams {
  const float* q;       // [B][H][64] f32
  const bf16_t* k;      // [B][H][kv_T][64]
  const bf16_t* v;
  int H, kv_T;
  const int* pos;       // if non-null: keys = pos[b] + 1 (self attention), else T
  int T;
  float scale_log2e;
  bf16_t* out_bf16;     // FINAL: [B][H*64]
  float* part_o;        // partials [B][H][nsplit][64]
  float* part_ml;       // [B][H][nsplit][2]
  int lds_pad;          // dynamic LDS the blocks claim without using it: caps the blocks per CU (see ccx_whisper_decode)
  int stream_mode;      // cross attention only: 1 = dec_cross_stream_kernel (few waves, few bytes in flight per CU)
  // prompt prefill: rows (q / out index) != sequences (K/V index).  row_seq [rows] maps them (null: identity); rows_per_seq > 1
  // tells the cross attention that the rows of a sequence are consecutive, so that it can co-schedule them on one XCD
  const int* row_seq; int rows_per_seq;
  // fused query projection (small batches, ccx_launch_dec_cross_fused_q): q = LN(x + pending slabs) * Wq^T + bq computed by the
  // attention block itself instead of by a launch of its own.  Wq: the fragment-packed image dec_linear streams.
  const float* qx; const float* q_pend; int q_pend_n; long q_pend_stride; float* q_x_out;
  const float* q_ln_g; const float* q_ln_b; float q_eps;
  const bf16_t* q_W; const float* q_bias; int q_K;
  // set by a decode over a row -> window map (ccx_whisper_decode_rows): row_seq is then honoured by the streaming kernel too, and the
  // prefill kernels take a group's sequence from row_seq instead of from the block index (the mapped instantiations).  The split-KV
  // kernel reads row_seq either way.  (Last, in the struct's tail padding: no other field moves.)
  int kv_map;
  // beam search (ccx_whisper_decode_beam): self attention through a cache indirection -- key t of row r is read from cache slot
  // ind[r * ind_ld + t] instead of slot r (dec_attention_kernel<true, true>).  Null: the unflagged kernels.  (Appended: no other
  // field moves; the kernel argument block of every attention kernel grows by these 16 bytes.)
  const unsigned short* ind; int ind_ld;
  // self attention of a decode step only (pos set, no row_seq, no ind; B a multiple of 16): out_bf16 is written as the fragment image
  // of the rows (dec_frag_off) instead of row-major (dec_attention_kernel<true, false, true>).  (Appended.)
  int out_packed;
};
int ccx_launch_dec_attention(ccx_ctx* ctx, const DecAttnParams& p, int B, int nsplit, bool final_out, hipStream_t stream);
// Cross attention of a small batch (B <= 16 rows) WITH its query projection: replaces ln_linear(Wcq) + ccx_launch_dec_attention(split
// partials).  Same arithmetic, operation for operation, as the two launches it replaces (q is bit-identical).
int ccx_launch_dec_cross_fused_q(ccx_ctx* ctx, const DecAttnParams& p, int B, int nsplit, hipStream_t stream);

struct DecSeqState {
  int pos, prompt_len, n_gen, done;
  int last_tok, pen_tok, last_ts_tok, n_tokens;
  float sum_logprob, no_speech_prob;
};

struct DecSelectParams {
  const float* logits; long ld_logits; int n_vocab;
  DecSeqState* state;
  const int* prompt; int max_prompt;
  int* cur_tok; int* pos;
  int* gen; int sample_len;
  int* n_done;
  const unsigned char* suppress_mask;  // [n_vocab rounded up to 4]
  int eot, blank, no_speech, timestamp_begin, max_initial_ts;
  // next-step embedding written by the select kernel: x[b] = tok_emb[next] + pos_emb[pos]
  const float* tok_emb; const float* pos_emb; float* x; int D;
  // sampling (GreedyDecoder.update with temperature > 0): sample_cfg = {float temperature, u32 seed_lo, u32 seed_hi, int top_k,
  // float top_p, float min_p, 0, 0} (8 words; the plain kernels read the first three) in
  // device memory (so that a captured step graph serves every temperature / seed); row0 = batch row of sequence 0 of
  // this launch (lanes), so that the noise of a sequence does not depend on how the batch is split
  const unsigned* sample_cfg; int row0;
  int sample;   // 0: greedy kernel (sample_cfg ignored); 1: kernel with the temperature > 0 branch
  const int* stream_id;   // sampling kernel only: [B] noise stream of every row instead of row0 + b (null: row0 + b)
  // decoding options (ccx_decode_options).  no_rules: the instantiations without ApplyTimestampRules (host side: which kernel is
  // launched); suppress_blank: those kernels ban rules.blank and eot on the first sampled step (the ruled kernels ban every text id
  // and eot there anyway and do not read it).  (Appended: no other field moves.)
  int no_rules, suppress_blank;
  // truncated sampling (ccx_decode_sampling_options; dec_truncate.h).  trunc: the TRUNC instantiations (host side: which kernel is
  // launched; needs sample); they read {int top_k, float top_p, float min_p} from sample_cfg[3 .. 5].  cut_out / kept_out /
  // kept_mass_out: device [B] or null (the model): the smallest kept logit, |K| and the mass of K, written by rows that sampled.
  // (Appended: no other field moves.)
  int trunc;
  float* cut_out; int* kept_out; float* kept_mass_out;
  // per-token log-probabilities (ccx_decode_logprob_options; dec_logprobs.h).  tok_logprob set: the LOGP instantiations (host side:
  // which kernel is launched).  A row that samples at step i = its n_gen stores the float it adds to sum_logprob in
  // tok_logprob[row][i] (device [B][sample_len]) and its top_n (id, log-probability) pairs in top_id / top_lp[row][i][0 .. top_n)
  // (device [B][sample_len][kLogprobMaxTop]; null allowed where top_n == 0).  Rows in the prompt phase and done rows write nothing.
  // (Appended: no other field moves.)
  float* tok_logprob; int* top_id; float* top_lp; int top_n;
};
constexpr int kLogprobMaxTop = CCX_LOGPROB_MAX_TOP;
int ccx_launch_dec_select(ccx_ctx* ctx, const DecSelectParams& p, int B, hipStream_t stream);

// Beam search head of a step (dec_beam.hip; openai-whisper decoding.py::BeamSearchDecoder.update restated in tests/beam_reference.py).
// Rows are grouped in windows of `beam` consecutive rows.  dec_beam_topk_kernel (one block per row) writes every row's top beam + 1
// (id, log-probability) pairs of the filtered logits; dec_beam_update_kernel (one block per window) ranks the window's candidates,
// walks them, and rewrites the rows in place: state, token history, cache-indirection rows, next embedding, finished tables.
constexpr int kBeamMax = 8;            // rows per window
constexpr int kBeamCandMax = 16;       // finished hypotheses kept per window (max_candidates)
struct DecBeamParams {
  DecSelectParams sel;                 // logits, state, cur_tok, pos, gen (= the rows' token histories), n_done, rules, embeddings
  int beam, max_cand;
  int* cand_id; float* cand_lp;        // [rows][beam + 1]: the proposals of this step (id -1: none)
  unsigned short* ind; int ind_ld;     // [rows][ind_ld] cache slots of every row's keys (absolute rows of the launch's row 0 = slot 0)
  int row0;                            // ... the slot of this launch's first row
  int* fin_tok; float* fin_score; int* fin_n; int* fin_count;   // [windows][max_cand][sample_len], [windows][max_cand] x 2, [windows]
  int* step_tok; int* step_parent;     // [rows] or null: this step's chosen token and source row (-1: the window did not step)
  // test aid (null: off), indexed [step = tokens sampled so far][row]: proposals, chosen (token, parent) and cumulative score
  int* tr_cand_id; float* tr_cand_lp; int* tr_tok; int* tr_parent; float* tr_score; int tr_rows;
};
int ccx_launch_dec_beam(ccx_ctx* ctx, const DecBeamParams& p, int n_windows, hipStream_t stream);

// The rules over a row's own sampled history (dec_history.hip: repetition_penalty, no_repeat_ngram_size), applied to the fp32 logit
// rows in place BEFORE the select / beam kernels: one block per row; rows that are done or in the prompt phase are not touched.
// gen [rows][sample_len] holds state[row].n_gen sampled ids; ids >= text_end (rules.eot) are never edited.
constexpr int kDecHistoryMax = 2048;   // ids of one row's history the block stages in LDS (sample_len <= it)
struct DecHistoryParams {
  float* logits; long ld;              // [rows][ld], edited in place
  const DecSeqState* state;            // [rows]
  const int* gen; int sample_len;
  int text_end;
  float penalty; int ngram;            // 1.0 / 0: off
};
int ccx_launch_dec_history(ccx_ctx* ctx, const DecHistoryParams& p, int rows, hipStream_t stream);

// The sequence bias (dec_bias.hip: sequence_bias / bad_words_ids / hotwords; the rule: include/ccx.h ccx_decode_bias_options), applied
// to the fp32 logit rows in place BEFORE the history rules: one block per row; rows that are done or in the prompt phase are not
// touched.  `tab` is the compiled table, kBiasTabInts ints of device memory at fixed offsets (floats as their bits):
//   [kBiasHdr ..)   header: {n1, n_keys, n_groups, n_multi}; the kernel reads every count from here, so a captured launch serves
//                   every table uploaded later
//   [kBiasL1Tgt ..) / [kBiasL1Bias ..)   the n1 distinct targets of the length-1 entries, ascending, and their sums b1
//   [kBiasKey ..)   the n_keys distinct LAST context ids of the longer entries, ascending;  [kBiasKeyOff ..) n_keys + 1 group offsets
//   [kBiasGrpTgt ..) one target per group (a group: one (key, target) pair);  [kBiasGrpOff ..) n_groups + 1 entry offsets
//   [kBiasEntLen ..) / [kBiasEntCtx ..) / [kBiasEntBias ..)   per entry, table order inside a group: context length L - 1, where its
//                   context starts in the pool, bias;  [kBiasCtx ..) the pool of context ids
constexpr int kBiasMaxEntries = 8192, kBiasMaxIds = 65536, kBiasMaxLen = 32;      // CCX_BIAS_MAX_* (static_assert in dec_bias.hip)
constexpr int kBiasHdr = 0;
constexpr int kBiasL1Tgt = 8;
constexpr int kBiasL1Bias = kBiasL1Tgt + kBiasMaxEntries;
constexpr int kBiasKey = kBiasL1Bias + kBiasMaxEntries;
constexpr int kBiasKeyOff = kBiasKey + kBiasMaxEntries;
constexpr int kBiasGrpTgt = kBiasKeyOff + kBiasMaxEntries + 8;
constexpr int kBiasGrpOff = kBiasGrpTgt + kBiasMaxEntries;
constexpr int kBiasEntLen = kBiasGrpOff + kBiasMaxEntries + 8;
constexpr int kBiasEntCtx = kBiasEntLen + kBiasMaxEntries;
constexpr int kBiasEntBias = kBiasEntCtx + kBiasMaxEntries;
constexpr int kBiasCtx = kBiasEntBias + kBiasMaxEntries;
constexpr int kBiasTabInts = kBiasCtx + kBiasMaxIds;
struct DecBiasParams {
  float* logits; long ld;              // [rows][ld], edited in place
  const DecSeqState* state;            // [rows]
  const int* gen; int sample_len;
  int text_end;
  const int* tab;                      // [kBiasTabInts]
};
int ccx_launch_dec_bias(ccx_ctx* ctx, const DecBiasParams& p, int rows, hipStream_t stream);
// Checks a caller's table and compiles it into `tab` (kBiasTabInts ints, host); `who` names the entry point in the messages.
// has_len1: whether any length-1 entry exists.  An empty table (opts null or n_entries == 0) compiles to a header of zeros.
int ccx_compile_bias_table(ccx_ctx* ctx, const char* who, const ccx_decode_bias_options* opts, int n_vocab, int text_end,
                           std::vector<int>& tab, bool* has_len1);
int ccx_launch_dec_embed(ccx_ctx* ctx, const float* tok_emb, const float* pos_emb, const int* cur_tok, const int* pos,
                         float* x, int B, int D, hipStream_t stream);
// Softmax of logit rows over the ids [lo, hi) only (dec_probs.hip; everything else counts as -inf): argmax[row] (lowest id on equal
// values), pick_prob[row] = probability of id `pick` (inside the range), and, if probs != nullptr, probs[row][hi - lo].
// logits [rows][ld] f32, 16-byte aligned, ld a multiple of 4 and >= hi; hi - (lo rounded down to 4) <= 53248.  All outputs on the device.
struct DecTokenProbsParams {
  const float* logits; long ld;
  int lo, hi, pick;
  int* argmax; float* pick_prob; float* probs;
};
int ccx_launch_dec_token_probs(ccx_ctx* ctx, const DecTokenProbsParams& p, int rows, hipStream_t stream);
// Probability of one picked id per row over the ids [0, hi) (dec_probs.hip, the row pass of the kernel above): out[row * out_stride] =
// softmax(logits[row][0 : hi])[picks[row * pick_stride]]; a row whose pick is negative is skipped (nothing loaded, nothing written).
// logits as above, hi <= 53248; picks (int32) and out (f32) on the device, every pick below hi (the caller checks).
struct DecPickProbsParams {
  const float* logits; long ld;
  int hi;
  const int* picks; long pick_stride;
  float* out; long out_stride;
};
int ccx_launch_dec_pick_probs(ccx_ctx* ctx, const DecPickProbsParams& p, int rows, hipStream_t stream);
// dst[i][:] = src[idx[i]][:] where idx[i] >= 0 (bf16 rows of D elements): the last prompt row of every sequence after a prefill pass
int ccx_launch_dec_gather_rows(ccx_ctx* ctx, const bf16_t* src, const int* idx, bf16_t* dst, int n, int D, hipStream_t stream);
int ccx_launch_dec_combine(ccx_ctx* ctx, const float* part_o, const float* part_ml, int nsplit, bf16_t* out, int M, int H,
                           hipStream_t stream);

// ---- host helpers shared by the model handle (whisper.hip) and the stand-alone operators (dec_ops.hip) -----------------------
// Weights of dec_linear_kernel / dec_cross_fused_q_kernel are stored MFMA-fragment-packed: tile (n/16, k/32) is 64 consecutive
// 16-byte chunks, chunk l = row n0 + (l & 15), columns k0 + 8*(l >> 4) .. +8.  Rows are zero padded to a multiple of `row_pad`.
static inline std::vector<bf16_t> pack_mfma_rows(const float* src, int N, int K, int row_pad) {
  const int Np = (N + row_pad - 1) / row_pad * row_pad;
  const int kst = K / 32;
  std::vector<bf16_t> tmp((size_t)Np * K, 0);
  for (int nt = 0; nt < Np / 16; nt++)
    for (int ks = 0; ks < kst; ks++)
      for (int l = 0; l < 64; l++) {
        const int n = nt * 16 + (l & 15), k0 = ks * 32 + 8 * (l >> 4);
        bf16_t* dst = &tmp[(((size_t)nt * kst + ks) * 64 + l) * 8];
        if (n < N)
          for (int j = 0; j < 8; j++) dst[j] = ccx_host_f32_to_bf16(src[(size_t)n * K + k0 + j]);
      }
  return tmp;
}

// The select kernel's suppress mask [V + 4] from the decode rules: SuppressTokens plus <|notimestamps|>, which ApplyTimestampRules
// bans at every step.  Checks the rule ids against the vocabulary; `who` is the entry point the messages name.
static inline int ccx_build_suppress_mask(ccx_ctx* ctx, const char* who, const ccx_decode_rules* r, int V, std::vector<unsigned char>& mask) {
  CCX_REQUIRE(ctx, r->eot >= 0 && r->eot < V, "%s: rules.eot = %d out of range [0, n_vocab = %d)", who, r->eot, V);
  CCX_REQUIRE(ctx, r->sot < V, "%s: rules.sot = %d out of range (n_vocab = %d)", who, r->sot, V);
  CCX_REQUIRE(ctx, r->no_speech < V, "%s: rules.no_speech = %d out of range (n_vocab = %d)", who, r->no_speech, V);
  CCX_REQUIRE(ctx, r->timestamp_begin <= V, "%s: rules.timestamp_begin = %d behind n_vocab = %d", who, r->timestamp_begin, V);
  CCX_REQUIRE(ctx, r->blank < V, "%s: rules.blank = %d out of range (n_vocab = %d)", who, r->blank, V);
  CCX_REQUIRE(ctx, r->no_timestamps < V, "%s: rules.no_timestamps = %d out of range (n_vocab = %d)", who, r->no_timestamps, V);
  mask.assign((size_t)V + 4, 0);
  for (int i = 0; i < r->n_suppress; i++) {
    CCX_REQUIRE(ctx, r->suppress[i] >= 0 && r->suppress[i] < V, "%s: rules.suppress[%d] = %d out of range [0, n_vocab = %d)", who, i, r->suppress[i], V);
    mask[r->suppress[i]] = 1;
  }
  if (r->no_timestamps >= 0) mask[r->no_timestamps] = 1;  // ApplyTimestampRules bans <|notimestamps|>
  return CCX_OK;
}

// The checks of ccx_decode_sampling_options (written so that a NaN fails them); `who` is the entry point the messages name.
static inline int ccx_check_sampling_options(ccx_ctx* ctx, const char* who, const ccx_decode_sampling_options* o) {
  CCX_REQUIRE(ctx, o->top_k >= 0, "%s: opts.top_k = %d is negative", who, o->top_k);
  CCX_REQUIRE(ctx, o->top_p > 0.f && o->top_p <= 1.f, "%s: opts.top_p = %g must lie in (0, 1]", who, (double)o->top_p);
  CCX_REQUIRE(ctx, o->min_p >= 0.f && o->min_p <= 1.f, "%s: opts.min_p = %g must lie in [0, 1]", who, (double)o->min_p);
  return CCX_OK;
}
// The check of ccx_decode_logprob_options; `who` is the entry point the messages name.
static inline int ccx_check_logprob_options(ccx_ctx* ctx, const char* who, const ccx_decode_logprob_options* o) {
  CCX_REQUIRE(ctx, o->top_n >= 0 && o->top_n <= CCX_LOGPROB_MAX_TOP, "%s: opts.top_n = %d out of range [0, %d]", who, o->top_n, CCX_LOGPROB_MAX_TOP);
  return CCX_OK;
}
// sample_cfg as the select kernels read it (DecSelectParams::sample_cfg)
static inline void ccx_fill_sample_cfg(unsigned (&cfg)[8], float temperature, uint64_t seed, const ccx_decode_sampling_options& s) {
  memset(cfg, 0, sizeof(cfg));
  memcpy(&cfg[0], &temperature, 4);
  cfg[1] = (unsigned)(seed & 0xffffffffu); cfg[2] = (unsigned)(seed >> 32);
  cfg[3] = (unsigned)s.top_k;
  memcpy(&cfg[4], &s.top_p, 4);
  memcpy(&cfg[5], &s.min_p, 4);
}

// Its sibling for a call's options (ccx_decode_options): the options' list instead of the rules' where one is given, and
// <|notimestamps|> only while the timestamp rules run -- without them upstream bans neither it nor the timestamp ids.  `r` carries
// the rules' own list; it is checked as above.
static inline int ccx_build_options_mask(ccx_ctx* ctx, const char* who, const ccx_decode_rules* r, const ccx_decode_options* o, int V,
                                         std::vector<unsigned char>& mask) {
  CCX_TRY(ccx_build_suppress_mask(ctx, who, r, V, mask));
  CCX_REQUIRE(ctx, o->without_timestamps == 0 || o->without_timestamps == 1, "%s: opts.without_timestamps = %d must be 0 or 1", who, o->without_timestamps);
  CCX_REQUIRE(ctx, o->suppress_blank == 0 || o->suppress_blank == 1, "%s: opts.suppress_blank = %d must be 0 or 1", who, o->suppress_blank);
  const int mi = o->max_initial_timestamp_index;
  CCX_REQUIRE(ctx, mi >= -2 && (mi < 0 || (r->timestamp_begin >= 0 && mi < V - r->timestamp_begin)),
              "%s: opts.max_initial_timestamp_index = %d out of range [-2, n_vocab - timestamp_begin = %d)", who, mi, V - r->timestamp_begin);
  CCX_REQUIRE(ctx, o->n_suppress >= 0 && (o->n_suppress == 0 || o->suppress), "%s: opts.n_suppress = %d with opts.suppress NULL", who, o->n_suppress);
  if (o->suppress) {
    mask.assign((size_t)V + 4, 0);
    for (int i = 0; i < o->n_suppress; i++) {
      CCX_REQUIRE(ctx, o->suppress[i] >= 0 && o->suppress[i] < V, "%s: opts.suppress[%d] = %d out of range [0, n_vocab = %d)", who, i, o->suppress[i], V);
      mask[o->suppress[i]] = 1;
    }
  }
  if (r->no_timestamps >= 0) {
    bool listed = false;                     // <|notimestamps|> in the list that holds (then it stays suppressed either way)
    const int n = o->suppress ? o->n_suppress : r->n_suppress;
    const int* l = o->suppress ? o->suppress : r->suppress;
    for (int i = 0; i < n; i++) listed |= l[i] == r->no_timestamps;
    mask[r->no_timestamps] = (listed || !o->without_timestamps) ? 1 : 0;
  }
  return CCX_OK;
}

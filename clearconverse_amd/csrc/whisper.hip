// whisper.hip -- Whisper model object of libccx: weight intake by openai-whisper state_dict names,
// encoder forward (conv stem as im2col MFMA GEMMs, 12 pre-LN transformer blocks, cross-KV
// projection) and greedy decoding (device-side state machine, step chain captured in a hipGraph).
//
// Replaces `self.whisper_model` of the reference (loaded at back/api.py:665-703, called at
// back/api.py:1286-1292, 1432-1438, 1474-1480).  Model semantics follow openai-whisper
// model.py / decoding.py [UPSTREAM-RECALL -- not vendored in the reference]; the CPU restatement
// the tests compare against is oracle/whisper_ref.py.
#include <algorithm>
#include <atomic>
#include <map>
#include <chrono>
#include <math.h>
#include <tuple>
#include "../../include/ccx.h"
#include "align.h"
#include "attention.h"
#include "ccx_common.h"
#include "cross_x.h"
#include "decoder.h"
#include "dec_head_row.h"
#include "elementwise.h"
#include "gemm_bf16.h"
#include "logmel.h"
#include "model_store.h"

namespace {

struct EncLayer {
  float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
  bf16_t *Wqkv, *Wo, *W1, *W2;
  float *bqkv, *bo, *b1, *b2;
};
struct DecLayer {
  float *ln1_g, *ln1_b, *lnc_g, *lnc_b, *ln2_g, *ln2_b;
  bf16_t *Wqkv, *Wo, *Wcq, *Wckv, *Wco, *W1, *W2;
  // the X-stream kernels' weights (cross_x.hip), each as the fragment image of its matrix (cross_x.h)
  bf16_t* WckT = nullptr;       // cross_attn.key.weight re-laid per head [H][D][64] for the expanded query
  bf16_t* Wcq_plain = nullptr;  // cross_attn.query.weight [D][D] (dec_xq_fused_kernel; Wcq is the same image padded to 16 rows: the same bytes)
  bf16_t* Wcv_x = nullptr;      // cross_attn.value.weight [D][D] (dec_xv_project_kernel; the row-major Wckv stays for project_cross_kv)
  // LayerNorm-free cross-attention query (dec_xq_lnfree_kernel): gamma folded into the weights, Wcq_g = gamma o Wcq (fragment
  // image), s_n = sum_k (gamma o Wcq)_nk over the bf16 values the MFMAs see, c_n = sum_k beta_k Wcq_nk + bcq_n
  bf16_t* Wcq_g = nullptr;
  float *scq = nullptr, *ccq = nullptr;
  // ... whose rows are centred by the row's attn_ln mean + mean(attn.out.bias) before the bf16 rounding where that mean exceeds the
  // row's std (DEPI_RESOLVE, centre_shift): the self-attention output adds mean(bias) + a part an offset of the stream does not move
  float bo_mean = 0.f;
  float *bqkv, *bo, *bcq, *bckv, *bco, *b1, *b2;
  bf16_t *crossK, *crossV, *selfK, *selfV;
};

// The mode of one decoder step (or prefill pass) of one lane, as a value -- and, being everything a captured step bakes in, the key
// of the step-graph cache.  Invariant: a field dec_step / dec_head branches on or passes by value is in the plan; anything else
// they read from the instance is constant between ccx_whisper_set_rules calls (weights, workspaces, dimensions, rule ids) -- the
// options' mask between the ccx_whisper_set_decode_options calls that change it, which drop the graphs of the plans that read it; the
// bias table's buffer keeps its address and the kernel reads its CONTENT, counts included, on the device, so no graph depends on it -- and
// what is neither (logits, counters, streams, per-call buffers) comes in through StepIo.
struct StepPlan {
  int b0, B;                      // the lane's rows [b0, b0 + B)
  int sample_len, max_prompt;
  int select;                     // the step ends in the select (or beam) kernel; 0: logits only
  int sampling;                   // temperature > 0: the sampling variant of the select kernel
  int cross_stream;               // 1 (decodes): lean-streaming cross attention (dec_cross_stream_kernel) for lanes > 16 rows;
                                  // 0 (teacher-forced passes): split-KV partials + dec_combine_kernel
  int cross_lds_pad;              // occupancy cap of the cross-attention blocks while lanes overlap (plan_lanes)
  int xs_active;                  // cross attention against the encoder output (select_cross_path)
  int lnfree, xs_fuse_q, fuse_cross_q, xs_full_lines, packed_act, packed_mid;   // the chain's form (read_chain_switches)
  int xs_fp8;                     // the X-stream reads the FP8 image (an FP8 instance, unless CCX_XS_FP8=0); 0 on a default instance
  int map_on, sid_on;             // the rows read a row -> window map / a stream-id table (ccx_whisper_decode_rows)
  int beam_size, beam_maxc;       // beam search (0: none) and its max_candidates
  int lane_idx;                   // whose stamp trace and stagger slot
  int stamp_level;                // diagnostic stamp nodes (0: none)
  int prefill_rows;               // P > 0: the prompt prefill pass over B sequences x P positions instead of a step
  // decoding options (ccx_whisper_set_decode_options; all 0 / the rules' index in a default decode)
  int opt_mask;                   // the head reads the options' suppress mask (w->opt_mask) instead of the rules'
  int no_ts;                      // without_timestamps: the select / beam kernels without ApplyTimestampRules
  int sup_blank;                  // suppress_blank as set (read by the no_ts kernels only)
  int max_init_ts;                // the max_initial_timestamp index the ruled kernels apply (< 0: rule off)
  // the rules over a row's own sampled history (ccx_whisper_set_history_options; both 0 in a default decode): dec_history_kernel
  // runs in front of the select / beam kernels when either is set
  int hist_ngram;                 // no_repeat_ngram_size
  int hist_pen_bits;              // repetition_penalty's float bits (0 when it is 1.0)
  // a sequence-bias table is set (ccx_whisper_set_bias_options; 0 in a default decode): dec_bias_kernel runs in front of
  // dec_history_kernel and the select / beam kernels.  The table itself is not in the plan: the kernel reads it through its header.
  int bias_on;
  // truncated sampling (ccx_whisper_set_sampling_options; 0 in a default decode): the select kernel's truncating instantiation.  Set
  // only with `sampling`, and only while one of the three values is off its default; the values themselves sit in sample_cfg.
  int trunc_on;
  // per-token log-probabilities (ccx_whisper_set_logprob_options; 0 in a default decode): 1 + top_n -- the select kernel's LOGP
  // instantiation, which takes top_n as a launch parameter
  int logp;
  auto tie() const {
    return std::tie(b0, B, sample_len, max_prompt, select, sampling, cross_stream, cross_lds_pad, xs_active, lnfree, xs_fuse_q, fuse_cross_q,
                    xs_full_lines, packed_act, packed_mid, map_on, sid_on, beam_size, beam_maxc, lane_idx, stamp_level, prefill_rows, opt_mask, no_ts, sup_blank,
                    max_init_ts, hist_ngram, hist_pen_bits, bias_on, trunc_on, xs_fp8, logp);
  }
  bool operator<(const StepPlan& o) const { return tie() < o.tie(); }
};
static_assert(sizeof(StepPlan) == 32 * sizeof(int) && std::tuple_size<decltype(StepPlan{}.tie())>::value == 32,
              "StepPlan: ints only, and every one of them in tie()");

}  // namespace

struct ccx_whisper {
  ccx_ctx* ctx = nullptr;
  ccx_whisper_dims d{};
  int max_batch = 0;
  bool finalized = false;
  ccx_whisper* scratch_donor = nullptr;   // ccx_whisper_share_encoder_scratch: log-mel / encoder workspaces of another instance
  int scratch_takers = 0;                 // instances that borrowed THIS instance's workspaces and are still alive
  bool destroy_pending = false;           // ccx_whisper_destroy was called while takers were alive: freed with the last taker
  std::atomic<ccx_whisper*> scratch_owner{nullptr};   // (donor) instance whose staged log-mel waits for its encode: a shared group has ONE user between logmel and encode
  hipEvent_t scratch_free = nullptr;      // (donor) recorded at the end of every encode of the group; every log-mel / set_mel of the
                                          // group waits for it, so that users of the shared workspaces are ordered on ANY streams
  ccx_dev_store store{"whisper"};          // staged tensors, the weight arena and every device allocation of the instance

  // derived sizes
  int Spad = 0;    // padded audio context (multiple of 128)
  int Vpad = 0;    // vocab rounded up to 128
  int V4 = 0;      // vocab rounded up to 4: what the select kernel runs on (ids [n_vocab, V4) are always suppressed)
  int Fraw = 3008; // frames computed by the log-mel pass (covers 30 s + reflect tail)
  static constexpr int kCrossSplitMax = 8;

  // tables
  LogmelTables lm{};
  // encoder weights
  bf16_t *Wc1 = nullptr, *Wc2 = nullptr;
  float *bc1 = nullptr, *bc2 = nullptr, *enc_pos = nullptr, *lnp_g = nullptr, *lnp_b = nullptr;
  std::vector<EncLayer> enc;
  // decoder weights
  float *tok_emb_f32 = nullptr, *dec_pos = nullptr, *lnd_g = nullptr, *lnd_b = nullptr;
  bf16_t* tok_emb_rm = nullptr;     // row-major [n_vocab][D] (logits through the tiled GEMM)
  std::vector<DecLayer> dec;
  // rules
  ccx_decode_rules rules{};
  unsigned char* suppress_mask = nullptr;
  bool rules_set = false;
  std::vector<int> rules_suppress;          // the rules' own list (rules.suppress points at the caller's array: not kept)
  // the call's options (ccx_whisper_set_decode_options) and their device mask; opts_on: they differ from the defaults
  ccx_decode_options opts{0, 1, -2, 0, nullptr};
  bool opts_on = false;
  unsigned char* opt_mask = nullptr;
  std::vector<unsigned char> opt_mask_host; // what opt_mask holds: a call that changes nothing keeps the option graphs
  // the call's history rules (ccx_whisper_set_history_options); {1.0, 0}: off, the plans and launches of a default decode
  ccx_decode_history_options hist{1.0f, 0};
  // the call's sequence-bias table (ccx_whisper_set_bias_options), compiled (decoder.h: kBiasTabInts ints); off: the plans and
  // launches of a default decode.  The buffer is allocated at the first non-empty table and keeps its address.
  bool bias_on = false;
  int* bias_tab = nullptr;
  // the call's truncated sampling (ccx_whisper_set_sampling_options); {0, 1.0, 0.0}: off, the plans and launches of a default decode
  ccx_decode_sampling_options trunc{0, 1.0f, 0.0f};
  // per-token log-probabilities (ccx_whisper_set_token_logprobs: the buffers, beside gen; ccx_whisper_set_logprob_options: the
  // call's top_n, -1 = off, the plans and launches of a default decode).  Off: nothing allocated.
  bool tok_logp = false;
  float *tok_lp = nullptr, *top_lp = nullptr;   // [max_batch][sample_cap], [max_batch][sample_cap][CCX_LOGPROB_MAX_TOP]
  int* top_id = nullptr;
  int logp_n = -1;
  int logp_R = 0, logp_SL = 0, logp_top = -1;   // the last decode: rows, sample_len and top_n it recorded with (-1: it did not)

  // workspaces (encoder)
  float* lm_raw = nullptr; unsigned int* lm_max = nullptr; int *lm_n = nullptr, *lm_seek = nullptr, *lm_seg = nullptr;
  bf16_t *im2col = nullptr, *h1 = nullptr, *xn = nullptr, *qb = nullptr, *kb = nullptr, *vtb = nullptr, *attn = nullptr,
         *ffn = nullptr, *xa = nullptr;
  float* x = nullptr;
  // workspaces (decoder)
  float *dx = nullptr, *dx2 = nullptr, *pend = nullptr, *dq = nullptr, *dlogits = nullptr, *part_o = nullptr, *part_ml = nullptr;
  bf16_t *dattn = nullptr, *dffn = nullptr, *dxn = nullptr;
  int *cur_tok = nullptr, *pos = nullptr, *prompt = nullptr, *gen = nullptr, *n_done = nullptr;
  unsigned* sample_cfg = nullptr;   // {temperature bits, seed lo, seed hi, top_k, top_p bits, min_p bits, 0, 0}: read by the select kernel every step
  DecSeqState* state = nullptr;
  int max_prompt_cap = 0, sample_cap = 0;
  // prompt prefill: one pass over every prompt position of every sequence (rows = sequence * P + position) instead of one
  // decode step per prompt token; row-indexed copies of the step buffers and the row tables
  static constexpr int kPrefillMax = 16;     // prompt positions prefilled in one pass (longer prompts: several passes)
  float *pf_x = nullptr, *pf_x2 = nullptr, *pf_pend = nullptr, *pf_q = nullptr;
  bf16_t *pf_xn = nullptr, *pf_attn = nullptr, *pf_ffn = nullptr;
  int *pf_tok = nullptr, *pf_pos = nullptr, *pf_seq = nullptr, *pf_last = nullptr;
  // decode over a row -> window map (ccx_whisper_decode_rows): row r keeps self-attention cache slot r and reads the cross K/V (or the
  // encoder output) of window row_win[r]; row_sid[r] is its noise stream.  Allocated by the first mapped decode; whether a step
  // reads them is in its plan.  pf_win: the prefill pass's row table composed with the map (row -> window).
  int *row_win = nullptr, *row_sid = nullptr, *pf_win = nullptr;
  int enc_B = 0;                             // windows of the last ccx_whisper_encode
  // beam search (ccx_whisper_decode_beam; dec_beam.hip).  Allocated by the first beam decode, sized from max_batch (a traced
  // call's buffers are its own: BeamTrace).  beam_ind [max_batch][n_text_ctx]: cache slot of every row's self-attention
  // keys; beam_cand_*: [max_batch][kBeamMax + 1] proposals of a step; beam_fin_*: the windows' finished hypotheses ([max_batch x
  // kBeamCandMax] slots: at beam_size 1 every row is a window).
  unsigned short* beam_ind = nullptr;
  int *beam_cand_id = nullptr, *beam_fin_tok = nullptr, *beam_fin_n = nullptr, *beam_fin_count = nullptr;
  float *beam_cand_lp = nullptr, *beam_fin_score = nullptr;
  // graph cache, keyed by the step plan; decode runs on an internal stream when the caller hands over the legacy null
  // stream (stream capture is illegal there)
  std::map<StepPlan, hipGraphExec_t> graphs;
  hipStream_t own_stream = nullptr;
  hipEvent_t own_event = nullptr;
  // decode lanes: disjoint row ranges of one batch stepping concurrently on their own streams, staggered so
  // that one lane's HBM-bound cross attention overlaps the other lanes' latency-bound linears.  The gain is
  // modest (3-4 % at 192 sequences): the small kernels slow down 3-5x while HBM is saturated by another lane.
  static constexpr int kMaxLanes = 4;
  // Cross attention against the encoder output (cross_x.hip) for decodes of more than 80 sequences: no per-layer K/V caches beyond those
  // (42 GB at 768 sequences), half the bytes per step.  xs_on: the instance was built for it (widths cross_x.hip instantiates,
  // CCX_CROSS_X != 0 at finalize); the K/V caches then hold kv_cap <= 80 sequences and are filled from xa at the start of a decode
  // that takes the K/V path (kv_ready = sequences valid since the last encode).
  static constexpr int kKvSeqs = 80;         // sequences the K/V caches of an X-stream instance hold (4.5 GB at small.en)
  bool xs_on = false;
  // FP8 encoder-output stream (ccx_whisper_set_cross_fp8, CCX_CROSS_FP8; cross_x.h): the image of xa that the X-stream reads, written by
  // the quantise kernel at the end of every encode, which also leaves xa holding the dequantised values.  Off: nothing allocated.
  bool cross_fp8 = false, cross_fp8_called = false;
  unsigned char* xa8 = nullptr;
  long xa8_stride = 0;                       // bytes between sequences
  // Reduced audio context (ccx_whisper_set_audio_ctx; include/ccx.h): ccx_whisper_encode_ctx keeps positions [0, n_ctx[b]) of window b,
  // xa_n holds the counts the X-stream reads (XsParams::seq_S), and every decode takes the X-stream path.  Off: nothing allocated.
  bool audio_ctx = false;
  int* xa_n = nullptr;                       // device [max_batch]: keys of every window of the last encode
  std::vector<int> enc_ctx;                  // the same on the host ([max_batch]; the alignment pass checks its windows against it)
  bool ctx_full = false;                     // xa_n holds n_audio_ctx everywhere
  int last_cross_path = -1;                  // ccx_whisper_last_cross_path: 0 kv16, 1 kv_stream, 2 xa_stream
  int kv_cap = 0, kv_ready = 0;
  bf16_t *xq = nullptr, *pf_xq = nullptr;    // expanded queries [rows][H][D] (step rows, prefill rows)
  // LayerNorm-free query of the X-stream path: bf16 copy of the resolved residual rows and their (sum, sum of squares) per 16-column tile
  bf16_t *dxb = nullptr, *pf_xb = nullptr;
  float2 *dst2 = nullptr, *pf_st2 = nullptr;
  float *dshift = nullptr, *pf_shift = nullptr;   // ... and the shift they are centred by (the attn_ln mean of the row)
  float *xs_po = nullptr, *xs_pml = nullptr, *pf_xs_po = nullptr, *pf_xs_pml = nullptr;   // key-half partials (cross_x.h)
  static constexpr int kLanePool = 8;
  hipStream_t lane_pool[kLanePool] = {};     // candidates; HIP streams share a few hardware queues and two streams on one
                                             // queue run strictly one after the other, so lanes are picked by a probe
  std::map<hipStream_t, std::vector<hipStream_t>> lane_sets;   // lane-0 stream -> streams that overlap with it and each other
  int* probe_sink = nullptr;
  unsigned long long* stamps = nullptr;      // [kMaxLanes][kStampCap] diagnostic trace (ccx_whisper_trace_lanes / CCX_DEC_STAMPS)
  int* stamp_count = nullptr;                // [kMaxLanes]
  bool stamps_on = false;                    // decodes run with plan.stamp_level = stamp_level while set, and append to stamp_path
  int stamp_level = 1;
  std::string stamp_path;
  static constexpr int kStampCap = 1 << 16;
  hipEvent_t lane_start[kMaxLanes] = {}, lane_poll[2][kMaxLanes] = {};
  int* poll_host = nullptr;                  // pinned [2][kMaxLanes]
  // word alignment (ccx_whisper_align; align.hip).  The workspaces are allocated by its first call, nothing at create / finalize.
  float *al_P = nullptr, *al_A = nullptr;    // [seqs][heads][T][n_audio_ctx], [seqs][T][n_audio_ctx]
  unsigned char* al_trace = nullptr;
  int* al_ints = nullptr;                    // tables of one call (heads, n_keys, rows) and its path / jump-frame outputs
  size_t al_P_elems = 0, al_A_elems = 0, al_trace_bytes = 0, al_ints_elems = 0;   // bytes held by each (own hipMallocs, freed at destroy)
  int* al_picks = nullptr;                   // ccx_whisper_align_probs only: [seqs][T] picked ids, then [seqs][T] f32 probabilities
  size_t al_picks_bytes = 0;
  // SOT sequences of more than one token, vocabularies that are no multiple of 4, language detection (dec_probs.hip).  The scratch
  // is allocated by the first call that needs it: an English-only instance allocates nothing and launches nothing for it.
  int sot_tail = 0;                          // ccx_whisper_set_sot_tail: tokens of the SOT sequence behind <|startoftranscript|>
  int prefix_len = 0;                        // ccx_whisper_set_prefix_len: prompt tokens behind the SOT sequence (DecodingOptions.prefix)
  static constexpr int kMaxLang = 128;       // ids of one ccx_whisper_detect_language range
  bf16_t* tp_xn = nullptr;                   // [max_batch][D]: final-LayerNorm row of every sequence's SOT position (run_prefill)
  int *tp_idx = nullptr, *tp_arg = nullptr;  // [max_batch]: that row in the prefill pass (or -1); the kernel's argmax
  float *tp_prob = nullptr, *tp_lang = nullptr;   // [max_batch]: the picked probability; [max_batch][kMaxLang]: the range's distribution
  bool ns_at_sot() const { return sot_tail + prefix_len > 0 || d.n_vocab % 4 != 0; }   // no_speech_prob comes from dec_token_probs_kernel
};

// the alignment pass in flight: which heads of which layer go where in P, and the token row the current step writes
struct AlignPass {
  std::vector<int> first, count;             // per decoder layer: range of its selected heads in the device tables
  const int *heads = nullptr, *hsel = nullptr, *n_keys = nullptr;   // device
  int Hsel = 0, T = 0, Mmax = 0, t = 0;
};

namespace {

// Decode-side weights are stored MFMA-fragment-packed for dec_linear_kernel (decoder.h pack_mfma_rows).
int up_bf16_packed(ccx_whisper* w, bf16_t** out, const float* src, int N, int K, int row_pad) {
  return w->store.upload(out, pack_mfma_rows(src, N, K, row_pad));
}

// conv weight [out][in][3] -> GEMM weight [out][Kpad] with k = tap*in + c
std::vector<float> conv_to_gemm(const ccx_host_tensor& t, int Kpad) {
  const int64_t O = t.shape[0], I = t.shape[1], T = t.shape[2];
  std::vector<float> r((size_t)O * Kpad, 0.f);
  for (int64_t o = 0; o < O; o++)
    for (int64_t c = 0; c < I; c++)
      for (int64_t k = 0; k < T; k++) r[(size_t)o * Kpad + k * I + c] = t.data[(o * I + c) * T + k];
  return r;
}

int build_logmel_tables(ccx_whisper* w) {
  CCX_NEED(w->store, mf, "mel_filters", w->d.n_mels, 201);
  const int NM = w->d.n_mels;
  CCX_REQUIRE(w->ctx, NM == 80 || NM == 128, "whisper: n_mels must be 80 or 128 (got %d)", NM);
  std::vector<float> c(400 * 208, 0.f), s(400 * 208, 0.f), fb((size_t)NM * 208, 0.f);
  std::vector<int> rg(2 * NM);
  const double two_pi = 6.283185307179586476925286766559;
  for (int n = 0; n < 400; n++) {
    const double win = 0.5 - 0.5 * cos(two_pi * n / 400.0);  // periodic Hann (torch.hann_window default)
    for (int k = 0; k < 201; k++) {
      const int ph = (int)(((long)n * k) % 400);  // exact phase reduction
      const double a = two_pi * ph / 400.0;
      c[n * 208 + k] = (float)(cos(a) * win);
      s[n * 208 + k] = (float)(sin(a) * win);
    }
  }
  for (int m = 0; m < NM; m++) {
    int k0 = 201, k1 = 0;
    for (int k = 0; k < 201; k++) {
      const float v = mf->data[m * 201 + k];
      fb[m * 208 + k] = v;
      if (v != 0.f) { if (k < k0) k0 = k; k1 = k + 1; }
    }
    if (k1 == 0) { k0 = 0; k1 = 0; }
    rg[2 * m] = k0; rg[2 * m + 1] = k1;
  }
  float *dc, *ds, *dfb; int* drg;
  CCX_TRY(w->store.upload(&dc, c));
  CCX_TRY(w->store.upload(&ds, s));
  CCX_TRY(w->store.upload(&dfb, fb));
  CCX_TRY(w->store.upload(&drg, rg));
  w->lm.dft_cos = dc; w->lm.dft_sin = ds; w->lm.mel_fb = dfb; w->lm.mel_range = drg; w->lm.n_mels = NM;
  return CCX_OK;
}

std::vector<float> cat_rows(std::initializer_list<const std::vector<float>*> parts) {
  std::vector<float> r;
  for (auto p : parts) r.insert(r.end(), p->begin(), p->end());
  return r;
}

// only_options: the graphs whose steps read the options' mask (a default decode's graphs stay)
void drop_graphs(ccx_whisper* w, bool only_options = false) {
  for (auto it = w->graphs.begin(); it != w->graphs.end();) {
    if (only_options && !it->first.opt_mask) { ++it; continue; }
    hipGraphExecDestroy(it->second);
    it = w->graphs.erase(it);
  }
}

// the legacy null stream handed over: order after everything queued on it, then run on the instance's own stream
int own_stream_if_null(ccx_whisper* w, hipStream_t* stream) {
  if (*stream) return CCX_OK;
  CCX_HIP(w->ctx, hipEventRecord(w->own_event, nullptr));
  CCX_HIP(w->ctx, hipStreamWaitEvent(w->own_stream, w->own_event, 0));
  *stream = w->own_stream;
  return CCX_OK;
}

}  // namespace

extern "C" {

int ccx_whisper_create(ccx_ctx* ctx, const ccx_whisper_dims* dims, int max_batch, ccx_whisper** out) {
  if (!ctx) return CCX_ERR_ARG;
  CCX_REQUIRE(ctx, dims && out, "ccx_whisper_create: null argument");
  CCX_REQUIRE(ctx, max_batch >= 1 && max_batch <= 1536, "ccx_whisper_create: max_batch %d out of range", max_batch);
  const ccx_whisper_dims& d = *dims;
  CCX_REQUIRE(ctx, d.n_audio_state % 128 == 0 && d.n_text_state == d.n_audio_state, "whisper: n_state must be a multiple of 128 and equal for encoder/decoder");
  CCX_REQUIRE(ctx, d.n_audio_state / d.n_audio_head == 64 && d.n_text_state / d.n_text_head == 64, "whisper: head_dim must be 64");
  CCX_REQUIRE(ctx, d.n_audio_state <= 1280, "whisper: n_state = %d exceeds the supported maximum of 1280", d.n_audio_state);
  CCX_REQUIRE(ctx, d.n_audio_ctx == 1500, "whisper: n_audio_ctx must be 1500 (got %d)", d.n_audio_ctx);
  CCX_REQUIRE(ctx, d.n_mels == 80 || d.n_mels == 128, "whisper: n_mels must be 80 or 128 (got %d)", d.n_mels);
  CCX_REQUIRE(ctx, d.n_audio_layer >= 1 && d.n_text_layer >= 1, "whisper: n_audio_layer = %d and n_text_layer = %d must be at least 1", d.n_audio_layer, d.n_text_layer);
  CCX_REQUIRE(ctx, d.n_audio_ctx % 4 == 0, "whisper: n_audio_ctx must be a multiple of 4");
  CCX_REQUIRE(ctx, d.n_vocab >= 4 && d.n_vocab <= kHeadMaxVocab, "whisper: n_vocab = %d out of range [4, 53248]", d.n_vocab);
  ccx_whisper* w = new ccx_whisper();
  w->ctx = ctx;
  w->store.ctx = ctx;
  w->store.zero_uploads = false;   // weight blocks get their copy only, no memset each (the workspaces pass zero = true)
  w->d = d;
  w->max_batch = max_batch;
  w->Spad = ccx_cdiv(d.n_audio_ctx, 128) * 128;
  w->Vpad = ccx_cdiv(d.n_vocab, 128) * 128;
  w->V4 = ccx_cdiv(d.n_vocab, 4) * 4;
  *out = w;
  return CCX_OK;
}

void ccx_whisper_destroy(ccx_whisper* w) {
  if (!w) return;
  if (w->scratch_takers > 0) {      // a taker still points into this instance's workspaces: keep everything until it is gone
    w->destroy_pending = true;
    return;
  }
  if (ccx_whisper* dn = w->scratch_donor) {
    w->scratch_donor = nullptr;
    ccx_whisper* me = w;
    dn->scratch_owner.compare_exchange_strong(me, nullptr);     // staged windows of a destroyed instance bind nobody
    if (--dn->scratch_takers == 0 && dn->destroy_pending) ccx_whisper_destroy(dn);
  }
  if (w->scratch_free) hipEventDestroy(w->scratch_free);
  drop_graphs(w);
  if (w->own_stream) hipStreamDestroy(w->own_stream);
  if (w->own_event) hipEventDestroy(w->own_event);
  for (int i = 0; i < ccx_whisper::kMaxLanes; i++) {
    if (w->lane_start[i]) hipEventDestroy(w->lane_start[i]);
    if (w->lane_poll[0][i]) hipEventDestroy(w->lane_poll[0][i]);
    if (w->lane_poll[1][i]) hipEventDestroy(w->lane_poll[1][i]);
  }
  for (int i = 0; i < ccx_whisper::kLanePool; i++)
    if (w->lane_pool[i]) hipStreamDestroy(w->lane_pool[i]);
  if (w->poll_host) hipHostFree(w->poll_host);
  for (void* p : {(void*)w->al_P, (void*)w->al_A, (void*)w->al_trace, (void*)w->al_ints, (void*)w->al_picks})
    if (p) hipFree(p);
  w->store.free_all();
  delete w;
}

int ccx_whisper_set_tensor(ccx_whisper* w, const char* name, const void* data, int dtype, int ndim, const int64_t* shape) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, !w->finalized, "whisper: set_tensor after finalize");
  CCX_REQUIRE(w->ctx, name && data && ndim >= 1 && ndim <= 4 && shape, "whisper: set_tensor bad arguments");
  const std::string nm(name);
  const bool known = nm == "mel_filters" || nm.rfind("encoder.", 0) == 0 || nm.rfind("decoder.", 0) == 0;
  CCX_REQUIRE(w->ctx, known, "whisper: unknown tensor name '%s'", name);
  return w->store.stage(name, data, dtype, ndim, shape);
}

int ccx_whisper_set_max_audio(ccx_whisper* w, double seconds) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, !w->finalized, "whisper: set_max_audio after finalize");
  CCX_REQUIRE(w->ctx, seconds >= 1.0 && seconds <= 7200.0, "whisper: max audio %.1f s out of range [1, 7200]", seconds);
  const long frames = (long)(seconds * 100.0) + 8;
  w->Fraw = (int)((frames + 31) / 32 * 32);
  if (w->Fraw < 3008) w->Fraw = 3008;
  return CCX_OK;
}

int ccx_whisper_set_cross_fp8(ccx_whisper* w, int on) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, !w->finalized, "whisper: set_cross_fp8 after finalize");
  if (on) {
    const ccx_whisper_dims& d = w->d;
    CCX_REQUIRE(w->ctx, d.n_text_state == d.n_audio_state && d.n_text_head == d.n_audio_head,
                "whisper: set_cross_fp8: decoder width %d (%d heads) differs from the encoder's %d (%d heads): the instance has no X-stream path",
                d.n_text_state, d.n_text_head, d.n_audio_state, d.n_audio_head);
    CCX_REQUIRE(w->ctx, ccx_xs_supported(d.n_audio_state, d.n_audio_head),
                "whisper: set_cross_fp8: width %d is not one the X-stream cross attention is instantiated for (128, 256, 384, 512, 768)", d.n_audio_state);
    const char* e = getenv("CCX_CROSS_X");
    CCX_REQUIRE(w->ctx, !e || atoi(e) != 0, "whisper: set_cross_fp8: CCX_CROSS_X=0 turns the X-stream path off, which is the only reader of the FP8 image");
  }
  w->cross_fp8 = on != 0;
  w->cross_fp8_called = true;
  return CCX_OK;
}

int ccx_whisper_cross_fp8(ccx_whisper* w) { return w && w->cross_fp8 ? 1 : 0; }

int ccx_whisper_set_token_logprobs(ccx_whisper* w, int on) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, !w->finalized, "whisper: set_token_logprobs after finalize");
  w->tok_logp = on != 0;
  return CCX_OK;
}

int ccx_whisper_set_audio_ctx(ccx_whisper* w, int on) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, !w->finalized, "whisper: set_audio_ctx after finalize");
  if (on) {      // the rule of ccx_whisper_set_cross_fp8: the X-stream is the only cross attention that reads a count per sequence
    const ccx_whisper_dims& d = w->d;
    CCX_REQUIRE(w->ctx, d.n_text_state == d.n_audio_state && d.n_text_head == d.n_audio_head,
                "whisper: set_audio_ctx: decoder width %d (%d heads) differs from the encoder's %d (%d heads): the instance has no X-stream path",
                d.n_text_state, d.n_text_head, d.n_audio_state, d.n_audio_head);
    CCX_REQUIRE(w->ctx, ccx_xs_supported(d.n_audio_state, d.n_audio_head),
                "whisper: set_audio_ctx: width %d is not one the X-stream cross attention is instantiated for (128, 256, 384, 512, 768)", d.n_audio_state);
    const char* e = getenv("CCX_CROSS_X");
    CCX_REQUIRE(w->ctx, !e || atoi(e) != 0, "whisper: set_audio_ctx: CCX_CROSS_X=0 turns the X-stream path off, which is the only cross attention with a key count per sequence");
    CCX_REQUIRE(w->ctx, d.n_audio_ctx >= 64, "whisper: set_audio_ctx: n_audio_ctx = %d is below the smallest context, 64", d.n_audio_ctx);
  }
  w->audio_ctx = on != 0;
  return CCX_OK;
}

int ccx_whisper_audio_ctx(ccx_whisper* w) { return w && w->audio_ctx ? 1 : 0; }

int ccx_whisper_share_encoder_scratch(ccx_whisper* w, ccx_whisper* donor) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, donor && donor != w && donor->finalized && !w->finalized, "whisper: share_encoder_scratch needs a finalized donor and an unfinalized taker");
  CCX_REQUIRE(w->ctx, donor->max_batch >= w->max_batch && donor->Fraw >= w->Fraw && !memcmp(&donor->d, &w->d, sizeof(w->d)),
              "whisper: share_encoder_scratch: the donor must have the same dimensions and at least the taker's capacity");
  if (!donor->scratch_free) CCX_HIP(w->ctx, hipEventCreateWithFlags(&donor->scratch_free, hipEventDisableTiming));
  w->scratch_donor = donor;
  donor->scratch_takers++;
  return CCX_OK;
}

int ccx_whisper_set_rules(ccx_whisper* w, const ccx_decode_rules* r) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, r, "whisper: rules null");
  const int V = w->d.n_vocab;
  std::vector<unsigned char> mask;
  CCX_TRY(ccx_build_suppress_mask(w->ctx, "ccx_whisper_set_rules", r, V, mask));
  // The select kernel runs on V4 ids: those behind the vocabulary never win or count.  Invariant: dec_select_kernel applies the mask
  // with a select (`allowed ? val : -inf`), never with arithmetic, so whatever the logit columns [n_vocab, V4) hold cannot leak into a
  // filtered quantity -- and they hold finite values anyway: the logits GEMM stores whole 16-column groups, up to n_vocab rounded up
  // to 16, from weight rows clamped to n_vocab - 1 (gemm_bf16.hip).  Only the kernel's own no-speech softmax reads them unmasked,
  // which is why that value is replaced (ns_at_sot).
  for (int v = V; v < w->V4; v++) mask[v] = 1;
  if (!w->suppress_mask) CCX_TRY(w->store.alloc(&w->suppress_mask, (size_t)V + 4, false));
  CCX_HIP(w->ctx, hipMemcpy(w->suppress_mask, mask.data(), (size_t)V + 4, hipMemcpyHostToDevice));
  w->rules = *r;
  w->rules_suppress.assign(r->suppress, r->suppress + (r->n_suppress > 0 ? r->n_suppress : 0));
  w->rules.suppress = nullptr;
  w->rules_set = true;
  w->opts = ccx_decode_options{0, 1, -2, 0, nullptr};   // the options name ids of the rules they were set under
  w->opts_on = false;
  w->hist = ccx_decode_history_options{1.0f, 0};
  w->bias_on = false;  // the table's targets were checked against the eot of the rules it was set under
  w->trunc = ccx_decode_sampling_options{0, 1.0f, 0.0f};
  w->logp_n = -1;
  drop_graphs(w);      // captured step graphs bake the rule ids into the select kernel's parameters
  return CCX_OK;
}

int ccx_whisper_graph_count(ccx_whisper* w, int options_only) {
  if (!w) return -1;
  int n = 0;
  for (auto& g : w->graphs) n += (!options_only || g.first.opt_mask) ? 1 : 0;
  return n;
}

void ccx_decode_options_default(ccx_decode_options* o) {
  if (o) *o = ccx_decode_options{0, 1, -2, 0, nullptr};
}

int ccx_whisper_set_decode_options(ccx_whisper* w, const ccx_decode_options* opts) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->rules_set, "ccx_whisper_set_decode_options: the rules are not set (ccx_whisper_set_rules)");
  ccx_decode_options o{0, 1, -2, 0, nullptr};
  if (opts) o = *opts;
  const int V = w->d.n_vocab;
  ccx_decode_rules r = w->rules;
  r.suppress = w->rules_suppress.data();
  std::vector<unsigned char> mask;
  CCX_TRY(ccx_build_options_mask(ctx, "ccx_whisper_set_decode_options", &r, &o, V, mask));
  for (int v = V; v < w->V4; v++) mask[v] = 1;     // as ccx_whisper_set_rules: the select kernel runs on V4 ids
  // suppress_blank alone changes nothing under the rules (the first step bans every text id and eot anyway): still a default decode
  const bool on = o.without_timestamps != 0 || o.suppress != nullptr ||
                  (o.max_initial_timestamp_index != -2 && o.max_initial_timestamp_index != w->rules.max_initial_timestamp_index);
  if (on && mask != w->opt_mask_host) {
    if (!w->opt_mask) CCX_TRY(w->store.alloc(&w->opt_mask, (size_t)V + 4, false));
    drop_graphs(w, true);                          // the option plans' graphs: their head reads this mask (a default decode's stay)
    CCX_HIP(ctx, hipMemcpy(w->opt_mask, mask.data(), (size_t)V + 4, hipMemcpyHostToDevice));
    w->opt_mask_host = mask;
  }
  w->opts = o;
  w->opts.suppress = nullptr; w->opts.n_suppress = 0;   // the list lives in the mask
  w->opts_on = on;
  return CCX_OK;
}

int ccx_whisper_set_history_options(ccx_whisper* w, const ccx_decode_history_options* opts) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->rules_set, "ccx_whisper_set_history_options: the rules are not set (ccx_whisper_set_rules)");
  ccx_decode_history_options o{1.0f, 0};
  if (opts) o = *opts;
  CCX_REQUIRE(ctx, o.repetition_penalty > 0.f && o.repetition_penalty <= 3.4028234e38f,
              "ccx_whisper_set_history_options: opts.repetition_penalty = %g must be finite and > 0", (double)o.repetition_penalty);
  CCX_REQUIRE(ctx, o.no_repeat_ngram_size >= 0, "ccx_whisper_set_history_options: opts.no_repeat_ngram_size = %d is negative", o.no_repeat_ngram_size);
  w->hist = o;         // both values are in the step plan: nothing captured depends on the setting itself
  return CCX_OK;
}

int ccx_whisper_history_graph_count(ccx_whisper* w) {
  if (!w) return -1;
  int n = 0;
  for (auto& g : w->graphs) n += (g.first.hist_ngram || g.first.hist_pen_bits) ? 1 : 0;
  return n;
}

void ccx_decode_sampling_options_default(ccx_decode_sampling_options* o) {
  if (o) *o = ccx_decode_sampling_options{0, 1.0f, 0.0f};
}

int ccx_whisper_set_sampling_options(ccx_whisper* w, const ccx_decode_sampling_options* opts) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->rules_set, "ccx_whisper_set_sampling_options: the rules are not set (ccx_whisper_set_rules)");
  ccx_decode_sampling_options o{0, 1.0f, 0.0f};
  if (opts) o = *opts;
  CCX_TRY(ccx_check_sampling_options(ctx, "ccx_whisper_set_sampling_options", &o));
  w->trunc = o;        // uploaded with {temperature, seed} by every decode: nothing captured depends on the values
  return CCX_OK;
}

int ccx_whisper_sampling_graph_count(ccx_whisper* w) {
  if (!w) return -1;
  int n = 0;
  for (auto& g : w->graphs) n += g.first.trunc_on ? 1 : 0;
  return n;
}

int ccx_whisper_set_logprob_options(ccx_whisper* w, const ccx_decode_logprob_options* opts) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->rules_set, "ccx_whisper_set_logprob_options: the rules are not set (ccx_whisper_set_rules)");
  if (!opts) { w->logp_n = -1; return CCX_OK; }
  CCX_REQUIRE(ctx, w->tok_lp != nullptr, "ccx_whisper_set_logprob_options: opts.top_n = %d on an instance without the buffers (ccx_whisper_set_token_logprobs before finalize)", opts->top_n);
  CCX_TRY(ccx_check_logprob_options(ctx, "ccx_whisper_set_logprob_options", opts));
  w->logp_n = opts->top_n;       // in the step plan: nothing captured depends on the setting itself
  return CCX_OK;
}

int ccx_whisper_logprob_graph_count(ccx_whisper* w) {
  if (!w) return -1;
  int n = 0;
  for (auto& g : w->graphs) n += g.first.logp ? 1 : 0;
  return n;
}

int ccx_whisper_token_logprobs(ccx_whisper* w, int R, int sample_len, float* tok_lp_out, int top_n, int32_t* top_id_out, float* top_lp_out,
                               void* stream_) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  if (w->logp_top < 0) return ccx_fail(ctx, CCX_ERR_STATE, "ccx_whisper_token_logprobs: the last decode did not record log-probabilities (ccx_whisper_set_logprob_options)");
  CCX_REQUIRE(ctx, R == w->logp_R && sample_len == w->logp_SL, "ccx_whisper_token_logprobs: R = %d, sample_len = %d, the last decode had %d rows of %d", R,
              sample_len, w->logp_R, w->logp_SL);
  CCX_REQUIRE(ctx, tok_lp_out != nullptr, "ccx_whisper_token_logprobs: tok_lp_out is NULL");
  CCX_REQUIRE(ctx, top_n >= 0 && top_n <= w->logp_top, "ccx_whisper_token_logprobs: top_n = %d out of range [0, the last decode's %d]", top_n, w->logp_top);
  CCX_REQUIRE(ctx, top_n == 0 || (top_id_out && top_lp_out), "ccx_whisper_token_logprobs: top_n = %d with top_id_out or top_lp_out NULL", top_n);
  hipStream_t stream = (hipStream_t)stream_;
  const size_t n = (size_t)R * sample_len;
  CCX_HIP(ctx, hipMemcpyAsync(tok_lp_out, w->tok_lp, n * 4, hipMemcpyDeviceToHost, stream));
  if (top_n > 0) {
    // the device tables are [row][step][CCX_LOGPROB_MAX_TOP]: the first top_n of every step
    CCX_HIP(ctx, hipMemcpy2DAsync(top_id_out, (size_t)top_n * 4, w->top_id, (size_t)CCX_LOGPROB_MAX_TOP * 4, (size_t)top_n * 4, n, hipMemcpyDeviceToHost, stream));
    CCX_HIP(ctx, hipMemcpy2DAsync(top_lp_out, (size_t)top_n * 4, w->top_lp, (size_t)CCX_LOGPROB_MAX_TOP * 4, (size_t)top_n * 4, n, hipMemcpyDeviceToHost, stream));
  }
  CCX_HIP(ctx, hipStreamSynchronize(stream));
  return CCX_OK;
}

int ccx_whisper_set_bias_options(ccx_whisper* w, const ccx_decode_bias_options* opts) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->rules_set, "ccx_whisper_set_bias_options: the rules are not set (ccx_whisper_set_rules)");
  if (!opts || opts->n_entries == 0) { w->bias_on = false; return CCX_OK; }
  std::vector<int> tab;
  CCX_TRY(ccx_compile_bias_table(ctx, "ccx_whisper_set_bias_options", opts, w->d.n_vocab, w->rules.eot, tab, nullptr));
  if (!w->bias_tab) CCX_TRY(w->store.alloc(&w->bias_tab, (size_t)kBiasTabInts, false));
  // no decode is in flight between two calls; captured bias plans read the new table through the same buffer and its header
  CCX_HIP(ctx, hipMemcpy(w->bias_tab, tab.data(), (size_t)kBiasTabInts * sizeof(int), hipMemcpyHostToDevice));
  w->bias_on = true;
  return CCX_OK;
}

int ccx_whisper_bias_graph_count(ccx_whisper* w) {
  if (!w) return -1;
  int n = 0;
  for (auto& g : w->graphs) n += g.first.bias_on ? 1 : 0;
  return n;
}

int ccx_whisper_trace_lanes(ccx_whisper* w, const char* path, int level) {
  CCX_REQUIRE(w->ctx, w->finalized, "whisper: trace_lanes before finalize");
  w->stamps_on = path != nullptr && path[0] != 0;
  w->stamp_path = w->stamps_on ? path : "";
  w->stamp_level = level >= 2 ? 2 : 1;
  CCX_HIP(w->ctx, hipMemset(w->stamp_count, 0, ccx_whisper::kMaxLanes * 4));
  return CCX_OK;      // (the stamp level is in the step plan: traced and untraced step graphs live side by side)
}

int ccx_whisper_finalize(ccx_whisper* w) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, !w->finalized, "whisper: finalize called twice");
  CCX_HIP(w->ctx, hipSetDevice(w->ctx->device));
  const ccx_whisper_dims& d = w->d;
  const int D = d.n_audio_state, F = 4 * D, B = w->max_batch, S = d.n_audio_ctx, H = d.n_audio_head;
  // Weights and per-step decode buffers are carved from ONE large allocation (bump pointer, in
  // access order): large contiguous mappings keep the decode chain's weight stream on few, large
  // TLB entries and make consecutive kernels touch consecutive addresses.  The arena holds all weights
  // (bf16 copies + fp32 vectors/embedding) and the small decode buffers; what does not fit gets a hipMalloc of its own.
  CCX_TRY(w->store.open_arena((size_t)64 << 20));
  CCX_TRY(build_logmel_tables(w));

  // ---------------- encoder ----------------
  {
    CCX_NEED(w->store, c1w, "encoder.conv1.weight", D, d.n_mels, 3);
    CCX_NEED(w->store, c1b, "encoder.conv1.bias", D);
    CCX_NEED(w->store, c2w, "encoder.conv2.weight", D, D, 3);
    CCX_NEED(w->store, c2b, "encoder.conv2.bias", D);
    CCX_NEED(w->store, pe, "encoder.positional_embedding", S, D);
    CCX_NEED(w->store, lg, "encoder.ln_post.weight", D);
    CCX_NEED(w->store, lb, "encoder.ln_post.bias", D);
    std::vector<float> g1 = conv_to_gemm(*c1w, ccx_logmel_kpad(d.n_mels)), g2 = conv_to_gemm(*c2w, 3 * D);
    CCX_TRY(w->store.upload_bf16(&w->Wc1, g1));
    CCX_TRY(w->store.upload_bf16(&w->Wc2, g2));
    CCX_TRY(w->store.upload(&w->bc1, c1b->data.data(), D));
    CCX_TRY(w->store.upload(&w->bc2, c2b->data.data(), D));
    CCX_TRY(w->store.upload(&w->enc_pos, pe->data.data(), (size_t)S * D));
    CCX_TRY(w->store.upload(&w->lnp_g, lg->data.data(), D));
    CCX_TRY(w->store.upload(&w->lnp_b, lb->data.data(), D));
  }
  w->enc.resize(d.n_audio_layer);
  const std::vector<float> zerosD(D, 0.f);
  for (int l = 0; l < d.n_audio_layer; l++) {
    const std::string p = "encoder.blocks." + std::to_string(l) + ".";
    EncLayer& L = w->enc[l];
    CCX_NEED(w->store, qw, p + "attn.query.weight", D, D); CCX_NEED(w->store, qbias, p + "attn.query.bias", D);
    CCX_NEED(w->store, kw, p + "attn.key.weight", D, D);
    CCX_NEED(w->store, vw, p + "attn.value.weight", D, D); CCX_NEED(w->store, vbias, p + "attn.value.bias", D);
    CCX_NEED(w->store, ow, p + "attn.out.weight", D, D); CCX_NEED(w->store, obias, p + "attn.out.bias", D);
    CCX_NEED(w->store, l1g, p + "attn_ln.weight", D); CCX_NEED(w->store, l1b, p + "attn_ln.bias", D);
    CCX_NEED(w->store, m0w, p + "mlp.0.weight", F, D); CCX_NEED(w->store, m0b, p + "mlp.0.bias", F);
    CCX_NEED(w->store, m2w, p + "mlp.2.weight", D, F); CCX_NEED(w->store, m2b, p + "mlp.2.bias", D);
    CCX_NEED(w->store, l2g, p + "mlp_ln.weight", D); CCX_NEED(w->store, l2b, p + "mlp_ln.bias", D);
    std::vector<float> wqkv = cat_rows({&qw->data, &kw->data, &vw->data});
    std::vector<float> bqkv = cat_rows({&qbias->data, &zerosD, &vbias->data});
    CCX_TRY(w->store.upload_bf16(&L.Wqkv, wqkv)); CCX_TRY(w->store.upload(&L.bqkv, bqkv));
    CCX_TRY(w->store.upload_bf16(&L.Wo, ow->data)); CCX_TRY(w->store.upload(&L.bo, obias->data.data(), D));
    CCX_TRY(w->store.upload_bf16(&L.W1, m0w->data)); CCX_TRY(w->store.upload(&L.b1, m0b->data.data(), F));
    CCX_TRY(w->store.upload_bf16(&L.W2, m2w->data)); CCX_TRY(w->store.upload(&L.b2, m2b->data.data(), D));
    CCX_TRY(w->store.upload(&L.ln1_g, l1g->data.data(), D)); CCX_TRY(w->store.upload(&L.ln1_b, l1b->data.data(), D));
    CCX_TRY(w->store.upload(&L.ln2_g, l2g->data.data(), D)); CCX_TRY(w->store.upload(&L.ln2_b, l2b->data.data(), D));
  }

  // ---------------- decoder ----------------
  {
    CCX_NEED(w->store, te, "decoder.token_embedding.weight", d.n_vocab, D);
    CCX_NEED(w->store, pe, "decoder.positional_embedding", d.n_text_ctx, D);
    CCX_NEED(w->store, lg, "decoder.ln.weight", D);
    CCX_NEED(w->store, lb, "decoder.ln.bias", D);
    CCX_TRY(w->store.upload(&w->tok_emb_f32, te->data));
    CCX_TRY(w->store.upload_bf16(&w->tok_emb_rm, te->data.data(), (size_t)d.n_vocab * D));
    CCX_TRY(w->store.upload(&w->dec_pos, pe->data));
    CCX_TRY(w->store.upload(&w->lnd_g, lg->data.data(), D));
    CCX_TRY(w->store.upload(&w->lnd_b, lb->data.data(), D));
  }
  w->dec.resize(d.n_text_layer);
  const int Tc = d.n_text_ctx;
  {
    const char* e = getenv("CCX_CROSS_X");      // 0: round 2's per-layer cross K/V caches for every sequence (A/B)
    w->xs_on = (!e || atoi(e) != 0) && d.n_text_state == D && d.n_text_head == H && ccx_xs_supported(D, H);
    w->kv_cap = w->xs_on ? (B < ccx_whisper::kKvSeqs ? B : ccx_whisper::kKvSeqs) : B;
    // the FP8 stream: the setter's word, else CCX_CROSS_FP8 (the benchmark's A/B); the setter was refused where there is no X-stream
    // path, and CCX_CROSS_X may have changed since
    const char* f = getenv("CCX_CROSS_FP8");
    if (!w->cross_fp8_called) w->cross_fp8 = w->xs_on && f && atoi(f) != 0;
    CCX_REQUIRE(w->ctx, !w->cross_fp8 || w->xs_on, "whisper: the FP8 encoder-output stream needs the X-stream path (CCX_CROSS_X=0?)");
    CCX_REQUIRE(w->ctx, !w->audio_ctx || w->xs_on, "whisper: the reduced audio context needs the X-stream path (CCX_CROSS_X=0?)");
  }
  for (int l = 0; l < d.n_text_layer; l++) {
    const std::string p = "decoder.blocks." + std::to_string(l) + ".";
    DecLayer& L = w->dec[l];
    CCX_NEED(w->store, qw, p + "attn.query.weight", D, D); CCX_NEED(w->store, qbias, p + "attn.query.bias", D);
    CCX_NEED(w->store, kw, p + "attn.key.weight", D, D);
    CCX_NEED(w->store, vw, p + "attn.value.weight", D, D); CCX_NEED(w->store, vbias, p + "attn.value.bias", D);
    CCX_NEED(w->store, ow, p + "attn.out.weight", D, D); CCX_NEED(w->store, obias, p + "attn.out.bias", D);
    CCX_NEED(w->store, l1g, p + "attn_ln.weight", D); CCX_NEED(w->store, l1b, p + "attn_ln.bias", D);
    CCX_NEED(w->store, cqw, p + "cross_attn.query.weight", D, D); CCX_NEED(w->store, cqb, p + "cross_attn.query.bias", D);
    CCX_NEED(w->store, ckw, p + "cross_attn.key.weight", D, D);
    CCX_NEED(w->store, cvw, p + "cross_attn.value.weight", D, D); CCX_NEED(w->store, cvb, p + "cross_attn.value.bias", D);
    CCX_NEED(w->store, cow, p + "cross_attn.out.weight", D, D); CCX_NEED(w->store, cob, p + "cross_attn.out.bias", D);
    CCX_NEED(w->store, lcg, p + "cross_attn_ln.weight", D); CCX_NEED(w->store, lcb, p + "cross_attn_ln.bias", D);
    CCX_NEED(w->store, m0w, p + "mlp.0.weight", F, D); CCX_NEED(w->store, m0b, p + "mlp.0.bias", F);
    CCX_NEED(w->store, m2w, p + "mlp.2.weight", D, F); CCX_NEED(w->store, m2b, p + "mlp.2.bias", D);
    CCX_NEED(w->store, l2g, p + "mlp_ln.weight", D); CCX_NEED(w->store, l2b, p + "mlp_ln.bias", D);
    std::vector<float> wqkv = cat_rows({&qw->data, &kw->data, &vw->data});
    std::vector<float> bqkv = cat_rows({&qbias->data, &zerosD, &vbias->data});
    std::vector<float> wckv = cat_rows({&ckw->data, &cvw->data});
    std::vector<float> bckv = cat_rows({&zerosD, &cvb->data});
    CCX_TRY(up_bf16_packed(w, &L.Wqkv, wqkv.data(), 3 * D, D, 16)); CCX_TRY(w->store.upload(&L.bqkv, bqkv));
    CCX_TRY(up_bf16_packed(w, &L.Wo, ow->data.data(), D, D, 16)); CCX_TRY(w->store.upload(&L.bo, obias->data.data(), D));
    { double sb = 0.0; for (int k = 0; k < D; k++) sb += obias->data[k]; L.bo_mean = (float)(sb / D); }
    CCX_TRY(up_bf16_packed(w, &L.Wcq, cqw->data.data(), D, D, 16)); CCX_TRY(w->store.upload(&L.bcq, cqb->data.data(), D));
    CCX_TRY(w->store.upload_bf16(&L.Wckv, wckv)); CCX_TRY(w->store.upload(&L.bckv, bckv));
    CCX_TRY(up_bf16_packed(w, &L.Wco, cow->data.data(), D, D, 16)); CCX_TRY(w->store.upload(&L.bco, cob->data.data(), D));
    CCX_TRY(up_bf16_packed(w, &L.W1, m0w->data.data(), F, D, 16)); CCX_TRY(w->store.upload(&L.b1, m0b->data.data(), F));
    CCX_TRY(up_bf16_packed(w, &L.W2, m2w->data.data(), D, F, 16)); CCX_TRY(w->store.upload(&L.b2, m2b->data.data(), D));
    CCX_TRY(w->store.upload(&L.ln1_g, l1g->data.data(), D)); CCX_TRY(w->store.upload(&L.ln1_b, l1b->data.data(), D));
    CCX_TRY(w->store.upload(&L.lnc_g, lcg->data.data(), D)); CCX_TRY(w->store.upload(&L.lnc_b, lcb->data.data(), D));
    CCX_TRY(w->store.upload(&L.ln2_g, l2g->data.data(), D)); CCX_TRY(w->store.upload(&L.ln2_b, l2b->data.data(), D));
    if (w->xs_on) {
      const std::vector<float> wkt = ccx_xs_relay_key(ckw->data.data(), H, D);
      CCX_TRY(up_bf16_packed(w, &L.WckT, wkt.data(), H * D, 64, 16));
      L.Wcq_plain = L.Wcq;
      CCX_TRY(up_bf16_packed(w, &L.Wcv_x, cvw->data.data(), D, D, 16));
      // cross_attn_ln folded into the cross-attention query (the LayerNorm-free query of the X-stream path)
      std::vector<float> Wg, sv, cv;
      ccx_xs_fold_query_ln(lcg->data.data(), lcb->data.data(), cqw->data.data(), cqb->data.data(), D, Wg, sv, cv);
      CCX_TRY(up_bf16_packed(w, &L.Wcq_g, Wg.data(), D, D, 16)); CCX_TRY(w->store.upload(&L.scq, sv)); CCX_TRY(w->store.upload(&L.ccq, cv));
    }
    const size_t ck = (size_t)w->kv_cap * H * w->Spad * 64, sk = (size_t)B * H * Tc * 64;
    CCX_TRY(w->store.alloc(&L.crossK, ck, true)); CCX_TRY(w->store.alloc(&L.crossV, ck, true));
    CCX_TRY(w->store.alloc(&L.selfK, sk, true)); CCX_TRY(w->store.alloc(&L.selfV, sk, true));
  }
  w->store.staged.clear();

  // ---------------- workspaces ----------------
  // log-mel and encoder: only live between ccx_whisper_logmel and the end of ccx_whisper_encode (the cross-KV it leaves behind is
  // per instance), so two instances whose log-mel / encode calls are ordered on ONE stream may share them (32 GB at 768 windows)
  if (ccx_whisper* dn = w->scratch_donor) {
    w->lm_raw = dn->lm_raw; w->lm_max = dn->lm_max; w->lm_n = dn->lm_n; w->lm_seek = dn->lm_seek; w->lm_seg = dn->lm_seg;
    w->im2col = dn->im2col; w->h1 = dn->h1; w->x = dn->x; w->xn = dn->xn;
    w->qb = dn->qb; w->kb = dn->kb; w->vtb = dn->vtb; w->attn = dn->attn; w->ffn = dn->ffn;
  } else {
    CCX_TRY(w->store.alloc(&w->lm_raw, (size_t)B * d.n_mels * w->Fraw, true));
    CCX_TRY(w->store.alloc(&w->lm_max, (size_t)B, true));
    CCX_TRY(w->store.alloc(&w->lm_n, (size_t)B, true));
    CCX_TRY(w->store.alloc(&w->lm_seek, (size_t)B, true));
    CCX_TRY(w->store.alloc(&w->lm_seg, (size_t)B, true));
    CCX_TRY(w->store.alloc(&w->im2col, (size_t)B * 3000 * ccx_logmel_kpad(d.n_mels), true));
    CCX_TRY(w->store.alloc(&w->h1, ((size_t)B * 3002 + 2) * D, true));
    CCX_TRY(w->store.alloc(&w->x, (size_t)B * S * D, true));
    CCX_TRY(w->store.alloc(&w->xn, (size_t)B * S * D, true));
    CCX_TRY(w->store.alloc(&w->qb, (size_t)B * H * w->Spad * 64, true));
    CCX_TRY(w->store.alloc(&w->kb, (size_t)B * H * w->Spad * 64, true));
    CCX_TRY(w->store.alloc(&w->vtb, (size_t)B * H * 64 * w->Spad, true));
    CCX_TRY(w->store.alloc(&w->attn, (size_t)B * S * D, true));
    CCX_TRY(w->store.alloc(&w->ffn, (size_t)B * S * F, true));
  }

  // the encoder output stays with the instance: the decode streams it (cross_x.hip); + one key tile of slack
  CCX_TRY(w->store.alloc(&w->xa, ((size_t)B * S + 16) * D, true));
  if (w->cross_fp8) {       // + one key tile of slack as well; zeroed: the quantise kernel leaves the unused scale bytes alone
    w->xa8_stride = xa_fp8_seq_bytes(S, D);
    CCX_TRY(w->store.alloc(&w->xa8, (size_t)B * w->xa8_stride + xa_fp8_tile_bytes(D), true));
  }
  if (w->audio_ctx) {
    w->enc_ctx.assign(B, S);
    CCX_TRY(w->store.upload(&w->xa_n, w->enc_ctx));
    w->ctx_full = true;
  }
  if (w->xs_on) {
    CCX_TRY(w->store.alloc(&w->xq, (size_t)B * H * D, true));
    CCX_TRY(w->store.alloc(&w->pf_xq, (size_t)B * ccx_whisper::kPrefillMax * H * D, true));
    CCX_TRY(w->store.alloc(&w->xs_po, ccx_xs_part_o_elems(B, H, D), true));
    CCX_TRY(w->store.alloc(&w->xs_pml, ccx_xs_part_ml_elems(B), true));
    CCX_TRY(w->store.alloc(&w->pf_xs_po, ccx_xs_part_o_elems((size_t)B * ccx_whisper::kPrefillMax, H, D), true));
    CCX_TRY(w->store.alloc(&w->pf_xs_pml, ccx_xs_part_ml_elems((size_t)B * ccx_whisper::kPrefillMax), true));
    CCX_TRY(w->store.alloc(&w->dxb, (size_t)B * D, true));
    CCX_TRY(w->store.alloc(&w->pf_xb, (size_t)B * ccx_whisper::kPrefillMax * D, true));
    CCX_TRY(w->store.alloc(&w->dst2, (size_t)B * (D / 16), true));
    CCX_TRY(w->store.alloc(&w->pf_st2, (size_t)B * ccx_whisper::kPrefillMax * (D / 16), true));
    CCX_TRY(w->store.alloc(&w->dshift, (size_t)B, true));
    CCX_TRY(w->store.alloc(&w->pf_shift, (size_t)B * ccx_whisper::kPrefillMax, true));
  }
  CCX_TRY(w->store.alloc(&w->dx, (size_t)B * D, true));
  CCX_TRY(w->store.alloc(&w->dx2, (size_t)B * D, true));
  CCX_TRY(w->store.alloc(&w->pend, (size_t)4 * B * D, true));
  CCX_TRY(w->store.alloc(&w->dxn, (size_t)B * D, true));
  CCX_TRY(w->store.alloc(&w->dq, (size_t)B * D, true));
  CCX_TRY(w->store.alloc(&w->dattn, (size_t)B * D, true));
  CCX_TRY(w->store.alloc(&w->dffn, (size_t)B * F, true));
  CCX_TRY(w->store.alloc(&w->dlogits, (size_t)B * w->Vpad, true));
  CCX_TRY(w->store.alloc(&w->part_o, (size_t)B * H * ccx_whisper::kCrossSplitMax * 64, true));
  CCX_TRY(w->store.alloc(&w->part_ml, (size_t)B * H * ccx_whisper::kCrossSplitMax * 2, true));
  CCX_TRY(w->store.alloc(&w->cur_tok, (size_t)B, true));
  CCX_TRY(w->store.alloc(&w->pos, (size_t)B, true));
  CCX_TRY(w->store.alloc(&w->n_done, (size_t)ccx_whisper::kMaxLanes, true));
  CCX_TRY(w->store.alloc(&w->sample_cfg, (size_t)8, true));
  CCX_TRY(w->store.alloc(&w->state, (size_t)B, true));
  {
    const size_t R = (size_t)B * ccx_whisper::kPrefillMax;
    CCX_TRY(w->store.alloc(&w->pf_x, R * D, true)); CCX_TRY(w->store.alloc(&w->pf_x2, R * D, true)); CCX_TRY(w->store.alloc(&w->pf_pend, 4 * R * D, true));
    CCX_TRY(w->store.alloc(&w->pf_q, R * D, true)); CCX_TRY(w->store.alloc(&w->pf_xn, R * D, true)); CCX_TRY(w->store.alloc(&w->pf_attn, R * D, true));
    CCX_TRY(w->store.alloc(&w->pf_ffn, R * F, true));
    CCX_TRY(w->store.alloc(&w->pf_tok, R, true)); CCX_TRY(w->store.alloc(&w->pf_pos, R, true)); CCX_TRY(w->store.alloc(&w->pf_seq, R, true));
    CCX_TRY(w->store.alloc(&w->pf_last, (size_t)B, true));
  }
  w->max_prompt_cap = d.n_text_ctx;
  w->sample_cap = d.n_text_ctx;
  CCX_TRY(w->store.alloc(&w->prompt, (size_t)B * w->max_prompt_cap, true));
  CCX_TRY(w->store.alloc(&w->gen, (size_t)B * w->sample_cap, true));
  if (w->tok_logp) {
    CCX_TRY(w->store.alloc(&w->tok_lp, (size_t)B * w->sample_cap, false));
    CCX_TRY(w->store.alloc(&w->top_id, (size_t)B * w->sample_cap * CCX_LOGPROB_MAX_TOP, false));
    CCX_TRY(w->store.alloc(&w->top_lp, (size_t)B * w->sample_cap * CCX_LOGPROB_MAX_TOP, false));
  }
  // decode streams get the highest priority: when other work shares the GPU (the front end of the next batch on another
  // stream) the short, latency-bound chain kernels should get the next free wave slot.
  int prio_least = 0, prio_greatest = 0;
  CCX_HIP(w->ctx, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  CCX_HIP(w->ctx, hipStreamCreateWithPriority(&w->own_stream, hipStreamNonBlocking, prio_greatest));
  CCX_HIP(w->ctx, hipEventCreateWithFlags(&w->own_event, hipEventDisableTiming));
  for (int i = 0; i < ccx_whisper::kMaxLanes; i++) {
    CCX_HIP(w->ctx, hipEventCreateWithFlags(&w->lane_start[i], hipEventDisableTiming));
    CCX_HIP(w->ctx, hipEventCreateWithFlags(&w->lane_poll[0][i], hipEventDisableTiming));
    CCX_HIP(w->ctx, hipEventCreateWithFlags(&w->lane_poll[1][i], hipEventDisableTiming));
  }
  for (int i = 0; i < ccx_whisper::kLanePool; i++) CCX_HIP(w->ctx, hipStreamCreateWithPriority(&w->lane_pool[i], hipStreamNonBlocking, prio_greatest));
  CCX_TRY(w->store.alloc(&w->probe_sink, (size_t)64, true));
  // lane trace buffers (2 MB): always there so that ccx_whisper_trace_lanes can switch the trace on later
  CCX_TRY(w->store.alloc(&w->stamps, (size_t)ccx_whisper::kMaxLanes * ccx_whisper::kStampCap, true));
  CCX_TRY(w->store.alloc(&w->stamp_count, (size_t)ccx_whisper::kMaxLanes, true));
  if (const char* e = getenv("CCX_DEC_STAMPS")) {
    w->stamps_on = true;
    w->stamp_path = e;
    if (const char* l = getenv("CCX_DEC_STAMP_LEVEL")) w->stamp_level = atoi(l);
  }
  CCX_HIP(w->ctx, hipHostMalloc((void**)&w->poll_host, 2 * ccx_whisper::kMaxLanes * sizeof(int), 0));
  w->finalized = true;
  return CCX_OK;
}

// Shared log-mel / encoder workspaces (ccx_whisper_share_encoder_scratch): every user waits for the end of the group's previous
// encode before it writes them, on whatever stream it runs (a no-op when all users share one stream).  The event only orders a
// logmel behind the previous ENCODE: between an instance's logmel / set_mel and its encode the workspaces hold its staged windows, so
// the host must issue that pair back to back -- enforced here: another instance's logmel in between is refused (include/ccx.h).
static int scratch_acquire(ccx_whisper* w, hipStream_t stream) {
  ccx_whisper* root = w->scratch_donor ? w->scratch_donor : w;
  if (root->scratch_free) {
    ccx_whisper* owner = root->scratch_owner.load(std::memory_order_acquire);
    CCX_REQUIRE(w->ctx, owner == nullptr || owner == w,
                "whisper: the shared encoder workspaces hold another instance's staged windows -- issue its ccx_whisper_encode before this logmel / set_mel");
    root->scratch_owner.store(w, std::memory_order_release);
    CCX_HIP(w->ctx, hipStreamWaitEvent(stream, root->scratch_free, 0));
  }
  return CCX_OK;
}
static int scratch_release(ccx_whisper* w, hipStream_t stream) {
  ccx_whisper* root = w->scratch_donor ? w->scratch_donor : w;
  if (root->scratch_free) {
    CCX_HIP(w->ctx, hipEventRecord(root->scratch_free, stream));
    ccx_whisper* me = w;
    root->scratch_owner.compare_exchange_strong(me, nullptr, std::memory_order_acq_rel);
  }
  return CCX_OK;
}

int ccx_whisper_logmel(ccx_whisper* w, const float* audio, int64_t stride, const int* n_samples, const int* seek, int B,
                       float* mel_out, void* stream_) {
  return ccx_whisper_logmel_ex(w, audio, stride, n_samples, seek, nullptr, B, mel_out, stream_);
}

int ccx_whisper_logmel_ex(ccx_whisper* w, const float* audio, int64_t stride, const int* n_samples, const int* seek, const int* max_frames,
                          int B, float* mel_out, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  CCX_REQUIRE(w->ctx, w->finalized, "whisper: not finalized");
  CCX_REQUIRE(w->ctx, audio && n_samples && B >= 1 && B <= w->max_batch, "whisper_logmel: bad arguments (B=%d, max %d)", B, w->max_batch);
  CCX_TRY(scratch_acquire(w, stream));
  long fcomp = 32;
  for (int b = 0; b < B; b++) {
    CCX_REQUIRE(w->ctx, n_samples[b] >= 0 && n_samples[b] <= stride, "whisper_logmel: n_samples[%d]=%d exceeds stride", b, n_samples[b]);
    const int s = seek ? seek[b] : 0;
    // frames that touch audio content must lie inside the computed range
    const long need_frames = ((long)n_samples[b] + 200 + 159) / 160 + 1;
    CCX_REQUIRE(w->ctx, need_frames <= w->Fraw, "whisper_logmel: clip %d (%d samples) exceeds the configured maximum of %d frames (ccx_whisper_set_max_audio)", b, n_samples[b], w->Fraw);
    if (need_frames > fcomp) fcomp = need_frames;
    CCX_REQUIRE(w->ctx, s >= 0, "whisper_logmel: negative seek");
    CCX_REQUIRE(w->ctx, !max_frames || max_frames[b] >= 0, "ccx_whisper_logmel_ex: max_frames[%d] = %d is negative", b, max_frames ? max_frames[b] : 0);
  }
  // segment_size = min(N_FRAMES, content_frames - seek[, clip end - seek]), content_frames = n_samples // 160 (transcribe.py); the
  // kernel writes literal zeros behind it, which is pad_or_trim on the cropped mel
  std::vector<int> seg(B), sk(B);
  for (int b = 0; b < B; b++) {
    sk[b] = seek ? seek[b] : 0;
    int sl = n_samples[b] / 160 - sk[b];
    seg[b] = sl < 0 ? 0 : (sl > 3000 ? 3000 : sl);
    if (max_frames && max_frames[b] < seg[b]) seg[b] = max_frames[b];
  }
  CCX_HIP(w->ctx, hipMemcpyAsync(w->lm_n, n_samples, B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipMemcpyAsync(w->lm_seek, sk.data(), B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipMemcpyAsync(w->lm_seg, seg.data(), B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipStreamSynchronize(stream));  // host staging vectors go out of scope
  fcomp = (fcomp + 31) / 32 * 32;   // only frames that touch audio are computed; everything later is log10(1e-10)
  return ccx_launch_logmel(w->ctx, w->lm, audio, stride, w->lm_n, w->lm_seek, w->lm_seg, B, w->Fraw, (int)fcomp, w->lm_raw,
                           w->lm_max, mel_out, w->im2col, stream);
}

int ccx_whisper_set_mel(ccx_whisper* w, const float* mel, int B, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, w->finalized && mel && B >= 1 && B <= w->max_batch, "whisper_set_mel: bad arguments");
  CCX_TRY(scratch_acquire(w, (hipStream_t)stream_));
  return ccx_launch_mel_to_im2col(w->ctx, w->d.n_mels, mel, B, w->im2col, (hipStream_t)stream_);
}

// cross-attention K/V of sequences [0, n) for every decoder layer out of xa (head-major, not transposed: decode streams rows)
static int project_cross_kv(ccx_whisper* w, int n, hipStream_t stream) {
  const ccx_whisper_dims& d = w->d;
  const int D = d.n_audio_state, S = d.n_audio_ctx, H = d.n_audio_head;
  CCX_REQUIRE(w->ctx, n <= w->kv_cap, "whisper: cross K/V caches hold %d sequences, %d asked for", w->kv_cap, n);
  GemmParams p;
  for (int l = 0; l < d.n_text_layer; l++) {
    const DecLayer& L = w->dec[l];
    memset(&p, 0, sizeof(p));
    p.A = w->xa; p.lda = D; p.W = L.Wckv; p.ldw = D; p.M = n * S; p.N = 2 * D; p.K = D; p.bias = L.bckv;
    p.hk = L.crossK; p.hv = L.crossV; p.d_model = D; p.n_head = H; p.S = S; p.Spad = w->Spad; p.v_transposed = 0;
    p.first_block = 1;
    CCX_TRY(ccx_launch_gemm(w->ctx, EPI_HEADS, p, stream));
  }
  w->kv_ready = n;
  return CCX_OK;
}
// The switches of the decode chain's form, read per call (tests flip them) by BOTH entry points that run dec_step -- decodes and
// ccx_whisper_decoder_logits -- so that the teacher-forced logits always come from the chain a decode of the same size would run.
// CCX_FUSE_CROSS_Q=0: the two-launch cross-attention query of <= 16 rows; CCX_DEC_LNFREE=0: round 3's X-stream query;
// CCX_XS_FUSE_Q=0: that query as a launch of its own; CCX_XS_FULL_LINES=0: the streaming kernel's half-line loads (cross_x.h);
// CCX_DEC_PACKED_ACT=0: the > 16-row chain's LayerNorm and GELU rows row-major between its kernels (decoder.h); CCX_DEC_PACKED_MID=0:
// its attention outputs and the resolved rows of the LayerNorm-free query.
// CCX_XS_FP8=0: an FP8 instance streams its bf16 encoder output (the dequantised values: the same bits) instead of the image.
static void read_chain_switches(const ccx_whisper* w, StepPlan& p) {
  { const char* e = getenv("CCX_FUSE_CROSS_Q"); p.fuse_cross_q = e ? (atoi(e) != 0) : 1; }
  { const char* e = getenv("CCX_DEC_LNFREE"); p.lnfree = !(e && strcmp(e, "0") == 0); }
  { const char* e = getenv("CCX_XS_FUSE_Q"); p.xs_fuse_q = !e || atoi(e) != 0; }
  p.xs_full_lines = ccx_xs_full_lines_switch();
  p.packed_act = ccx_dec_packed_act_switch();
  p.packed_mid = ccx_dec_packed_mid_switch();
  { const char* e = getenv("CCX_XS_FP8"); p.xs_fp8 = w->cross_fp8 && (!e || atoi(e) != 0); }
}
// which cross attention a decode of B = p.B sequences uses (-> p.xs_active), and the K/V it needs
// (n_kv: the sequences whose K/V the rows read -- B itself, or the windows of a mapped decode)
static int select_cross_path(ccx_whisper* w, StepPlan& p, hipStream_t stream, int n_kv = -1) {
  const int B = p.B;
  // CCX_CROSS_X_MIN_ROWS (read per call: tests flip it): smallest decode that takes the X-stream path.  Default 81: the streaming kernel
  // runs two blocks per sequence, and below ~160 blocks they do not fill the chip -- Whisper only, 24 / 32 / 48 / 64 / 96 x 30 s:
  // 300.7 / 311.8 / 340.0 / 357.9 / 404.3 ms per batch on the X-stream path against 208.6 / 223.3 / 289.4 / 329.3 / 427.2 on per-layer
  // K / V (split-KV kernels with the fused query up to 16 sequences, the lean streaming kernel above).  Within one path a sequence's
  // numbers do not depend on its batch mates; across the paths they agree to rounding (tests/test_whisper_gpu.py).  Decodes the K / V
  // caches cannot hold (kv_cap sequences) always take the X-stream path.
  const char* e = getenv("CCX_CROSS_X_MIN_ROWS");
  const int min_rows = e ? atoi(e) : ccx_whisper::kKvSeqs + 1;
  if (n_kv < 0) n_kv = B;
  // a reduced-audio-context instance: always -- the K / V-cache kernels know no key count per sequence
  p.xs_active = w->xs_on && (w->audio_ctx || B >= min_rows || n_kv > w->kv_cap);
  if (w->xs_on && !p.xs_active && w->kv_ready < n_kv) CCX_TRY(project_cross_kv(w, n_kv, stream));
  return CCX_OK;
}
// the plan of a single lane of B rows whose cross attention runs uncapped (no other lane to leave room for): the chain switches of
// the call, one token per step.  What a caller's steps do differently is set at its call site.
static StepPlan single_lane_plan(const ccx_whisper* w, int B, int max_prompt) {
  StepPlan p{};
  p.B = B; p.sample_len = 1; p.max_prompt = max_prompt; p.cross_stream = 1;
  p.stamp_level = w->stamps_on ? w->stamp_level : 0;
  read_chain_switches(w, p);
  return p;
}

// the counts of the windows [0, B) to the device (n_ctx null: n_audio_ctx for every window of the instance)
static int upload_audio_ctx(ccx_whisper* w, const int* n_ctx, int B, hipStream_t stream) {
  if (!n_ctx && w->ctx_full) return CCX_OK;
  const int n = n_ctx ? B : w->max_batch;
  for (int b = 0; b < n; b++) w->enc_ctx[b] = n_ctx ? n_ctx[b] : w->d.n_audio_ctx;
  CCX_HIP(w->ctx, hipMemcpyAsync(w->xa_n, w->enc_ctx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipStreamSynchronize(stream));     // enc_ctx is written again by the next encode
  w->ctx_full = !n_ctx;
  return CCX_OK;
}

// n_ctx (host [B], or null: the whole window for every sequence): the encoder at S = max(n_ctx) rows per sequence, sequence b attending
// over its first n_ctx[b] positions (include/ccx.h, ccx_whisper_encode_ctx).  S = n_audio_ctx runs the launches of the plain encode.
static int encode_impl(ccx_whisper* w, int B, const int* n_ctx, float* xa_out, hipStream_t stream) {
  ccx_ctx* ctx = w->ctx;
  const ccx_whisper_dims& d = w->d;
  const int D = d.n_audio_state, F = 4 * D, Sfull = d.n_audio_ctx, H = d.n_audio_head;
  int S = Sfull;
  const int* n_keys = nullptr;       // device: the attention's count per sequence
  if (n_ctx) {
    S = 0;
    for (int b = 0; b < B; b++) S = n_ctx[b] > S ? n_ctx[b] : S;
    S = (S + 3) & ~3;                // the heads epilogue of the q | k | v GEMM stores V^T four rows at a time
    if (S > Sfull) S = Sfull;
    n_keys = w->xa_n;
  }
  if (w->audio_ctx) CCX_TRY(upload_audio_ctx(w, n_ctx, B, stream));
  GemmParams p;
  // conv1 + GELU: [B*3000,KP] x [D,KP]^T -> h1 rows b*3002 + 1 + t (KP = 256 for 80 mels, 384 for 128)
  const int KP = ccx_logmel_kpad(d.n_mels);
  memset(&p, 0, sizeof(p));
  p.A = w->im2col; p.lda = KP; p.W = w->Wc1; p.ldw = KP; p.M = B * 3000; p.N = D; p.K = KP;
  p.bias = w->bc1; p.out = w->h1; p.ldo = D; p.rpb_in = 3000; p.rpb_out = 3002; p.roff = 1; p.rpb_valid = 3000;
  CCX_TRY(ccx_launch_gemm(ctx, EPI_BF16_GELU, p, stream));
  // conv2 (stride 2) + GELU + positional embedding: row m' = b*1501 + t reads h1 rows 2m' .. 2m'+2
  memset(&p, 0, sizeof(p));
  p.A = w->h1; p.lda = 2 * D; p.W = w->Wc2; p.ldw = 3 * D; p.M = B * 1501; p.N = D; p.K = 3 * D;
  p.bias = w->bc2; p.out = w->x; p.ldo = D; p.resid = w->enc_pos; p.ldr = D; p.resid_mod = S;
  p.rpb_in = 1501; p.rpb_out = S; p.roff = 0; p.rpb_valid = S;
  CCX_TRY(ccx_launch_gemm(ctx, EPI_F32_GELU_POS, p, stream));   // (S < n_audio_ctx: the rows behind S are dropped by the row remap)

  const int M = B * S;
  for (int l = 0; l < d.n_audio_layer; l++) {
    const EncLayer& L = w->enc[l];
    CCX_TRY(ccx_launch_layernorm(ctx, w->x, D, L.ln1_g, L.ln1_b, w->xn, nullptr, D, M, D, 1e-5f, stream));
    memset(&p, 0, sizeof(p));
    p.A = w->xn; p.lda = D; p.W = L.Wqkv; p.ldw = D; p.M = M; p.N = 3 * D; p.K = D; p.bias = L.bqkv;
    p.hq = w->qb; p.hk = w->kb; p.hv = w->vtb; p.d_model = D; p.n_head = H; p.S = S; p.Spad = w->Spad; p.v_transposed = 1;
    CCX_TRY(ccx_launch_gemm(ctx, EPI_HEADS, p, stream));
    CCX_TRY(ccx_launch_enc_attention(ctx, w->qb, w->kb, w->vtb, w->attn, B, H, S, w->Spad, stream, n_keys));
    memset(&p, 0, sizeof(p));
    p.A = w->attn; p.lda = D; p.W = L.Wo; p.ldw = D; p.M = M; p.N = D; p.K = D; p.bias = L.bo;
    p.out = w->x; p.ldo = D; p.resid = w->x; p.ldr = D;
    CCX_TRY(ccx_launch_gemm(ctx, EPI_F32_RESID, p, stream));
    CCX_TRY(ccx_launch_layernorm(ctx, w->x, D, L.ln2_g, L.ln2_b, w->xn, nullptr, D, M, D, 1e-5f, stream));
    memset(&p, 0, sizeof(p));
    p.A = w->xn; p.lda = D; p.W = L.W1; p.ldw = D; p.M = M; p.N = F; p.K = D; p.bias = L.b1; p.out = w->ffn; p.ldo = F;
    CCX_TRY(ccx_launch_gemm(ctx, EPI_BF16_GELU, p, stream));
    memset(&p, 0, sizeof(p));
    p.A = w->ffn; p.lda = F; p.W = L.W2; p.ldw = F; p.M = M; p.N = D; p.K = F; p.bias = L.b2;
    p.out = w->x; p.ldo = D; p.resid = w->x; p.ldr = D;
    CCX_TRY(ccx_launch_gemm(ctx, EPI_F32_RESID, p, stream));
  }
  // xa keeps its slot stride of n_audio_ctx rows per window whatever S is: lane offsets, row maps, the FP8 image's stride and captured
  // step graphs stay what they are
  CCX_TRY(ccx_launch_layernorm_rows(ctx, w->x, D, w->lnp_g, w->lnp_b, w->xa, w->cross_fp8 ? nullptr : xa_out, D, M, D, 1e-5f, S == Sfull ? 0 : S,
                                    Sfull, stream));
  // FP8 instance: the image for the X-stream, and xa (and xa_out) become the dequantised values every consumer then shares.  All
  // n_audio_ctx rows of a slot, as always: the rows behind S are an earlier encode's (or zeros), finite, and no key of this one
  if (w->cross_fp8) CCX_TRY(ccx_launch_xa_fp8_quantise(ctx, w->xa, (long)Sfull * D, w->xa8, w->xa8_stride, xa_out, B, Sfull, D, stream));
  CCX_TRY(scratch_release(w, stream));
  w->enc_B = B;
  // cross-attention K/V: with the X-stream cross attention only decodes of <= 80 sequences use them and project them themselves
  w->kv_ready = 0;
  if (!w->xs_on) CCX_TRY(project_cross_kv(w, B, stream));
  return CCX_OK;
}

int ccx_whisper_encode(ccx_whisper* w, int B, float* xa_out, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, w->finalized, "whisper: not finalized");
  CCX_REQUIRE(w->ctx, B >= 1 && B <= w->max_batch, "whisper_encode: B=%d out of range (max %d)", B, w->max_batch);
  return encode_impl(w, B, nullptr, xa_out, (hipStream_t)stream_);
}

int ccx_whisper_encode_ctx(ccx_whisper* w, int B, const int* n_ctx, float* xa_out, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->finalized, "whisper: not finalized");
  CCX_REQUIRE(ctx, w->audio_ctx, "ccx_whisper_encode_ctx: the instance was not built for a reduced audio context (ccx_whisper_set_audio_ctx before finalize)");
  CCX_REQUIRE(ctx, B >= 1 && B <= w->max_batch, "ccx_whisper_encode_ctx: B = %d out of range [1, max_batch = %d]", B, w->max_batch);
  CCX_REQUIRE(ctx, n_ctx != nullptr, "ccx_whisper_encode_ctx: n_ctx is NULL");
  for (int b = 0; b < B; b++)
    CCX_REQUIRE(ctx, n_ctx[b] >= 64 && n_ctx[b] <= w->d.n_audio_ctx, "ccx_whisper_encode_ctx: n_ctx[%d] = %d out of range [64, n_audio_ctx = %d]", b, n_ctx[b],
                w->d.n_audio_ctx);
  return encode_impl(w, B, n_ctx, xa_out, (hipStream_t)stream_);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// decoder
// ---------------------------------------------------------------------------------------------
namespace {

// ---- diagnostic time stamps (CCX_DEC_STAMPS=<file>, CCX_DEC_STAMP_LEVEL=1|2) ----
// A one-thread kernel that appends the 100 MHz wall clock (s_memrealtime) and a tag to the lane's trace; captured into the step
// graphs like any other node.  Level 1 brackets the cross attention of every layer (tags 1 / 2), level 2 also stamps after every
// chain kernel (tag 16 + kernel index in the layer).  Perturbs what it measures (one more ~2 us node per stamp): level 1 adds 24
// nodes to a step of ~150, and is what tools/decode_stamps.py reads.
__global__ void dec_stamp_kernel(unsigned long long* trace, int* count, int cap, int tag) {
  const int i = atomicAdd(count, 1);
  if (i < cap) trace[i] = (__builtin_amdgcn_s_memrealtime() << 8) | (unsigned long long)(tag & 255);
}

// ---- lane stream selection ----
// HIP multiplexes streams onto a handful of hardware queues, and streams that share a queue execute strictly one
// after the other (tools/microbench_lanes2.hip: some pairs of 8 fresh streams take 2x, the others 1x).  The mapping
// is fixed when a stream is created but not queryable, so it is measured: a few ~50 us spin kernels per stream.
__global__ void lane_probe_spin(int* sink, long cycles) {
  const long t0 = __builtin_amdgcn_s_memtime();
  while (__builtin_amdgcn_s_memtime() - t0 < cycles) {}
  if (sink && threadIdx.x == 0) atomicAdd(sink, 1);
}

double lane_probe_time(ccx_whisper* w, hipStream_t a, hipStream_t b) {
  hipStreamSynchronize(a);
  if (b) hipStreamSynchronize(b);
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < 4; k++) {
    hipLaunchKernelGGL(lane_probe_spin, dim3(1), dim3(64), 0, a, w->probe_sink, 120000L);
    if (b) hipLaunchKernelGGL(lane_probe_spin, dim3(1), dim3(64), 0, b, w->probe_sink + 1, 120000L);
  }
  hipStreamSynchronize(a);
  if (b) hipStreamSynchronize(b);
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// streams (up to kMaxLanes - 1) that run concurrently with s0 and with each other; fewer if the probe finds fewer
const std::vector<hipStream_t>& lane_streams_for(ccx_whisper* w, hipStream_t s0) {
  auto it = w->lane_sets.find(s0);
  if (it != w->lane_sets.end()) return it->second;   // probed once per lane-0 stream (always for the maximum)
  std::vector<hipStream_t>& set = w->lane_sets[s0];
  set.clear();
  lane_probe_time(w, s0, nullptr);                        // warm-up (code object load)
  double single = lane_probe_time(w, s0, nullptr);
  const double s2 = lane_probe_time(w, s0, nullptr);
  if (s2 < single) single = s2;
  for (int c = 0; c < ccx_whisper::kLanePool && (int)set.size() < ccx_whisper::kMaxLanes - 1; c++) {
    hipStream_t cand = w->lane_pool[c];
    bool ok = lane_probe_time(w, s0, cand) < 1.5 * single;
    for (size_t j = 0; ok && j < set.size(); j++) ok = lane_probe_time(w, set[j], cand) < 1.5 * single;
    if (ok) set.push_back(cand);
  }
  if (getenv("CCX_DEBUG_LANES")) fprintf(stderr, "[lanes] probe: single %.0f us, %zu concurrent streams found\n", single, set.size());
  return set;
}

// key splits of the cross attention on the K/V caches
int cross_split(int B, int H, bool lean) {
  // lean streaming: one block owns the whole key range of a (sequence, head) -- 12 rolling 32-key pieces per wave, FINAL output,
  // no partials and no combine launch
  if (lean && B > 16) return 1;
  // enough blocks to fill the chip, and <= 256 keys per block (one 64-key chunk per wave).  Measured at 64 sequences per lane:
  // 6 splits 54.5 us per launch, 8 splits 56.8 us (a wave then owns 47 of a chunk's 64 keys).
  int ns = ccx_cdiv(512, B * H);
  if (ns < 6) ns = 6;
  if (ns > ccx_whisper::kCrossSplitMax) ns = ccx_whisper::kCrossSplitMax;
  return ns;
}

// device buffers of one traced beam decode: [steps][rows][beam + 1] proposals, [steps][rows] outcomes
struct BeamTrace {
  int *cid = nullptr, *tok = nullptr, *par = nullptr;
  float *clp = nullptr, *score = nullptr;
};

// What a step reads and writes that is not mode: where its logits go, the lane's done counter, its stream -- and the per-call
// buffers of the two kinds of step that are never captured (step_graph checks): ccx_whisper_align's pass and a traced beam decode.
struct StepIo {
  float* logits = nullptr;                   // row 0 = sequence plan.b0, row stride ld
  long ld = 0;
  int* n_done = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t stagger = nullptr;              // if set, recorded right before layer 0's cross attention
  const AlignPass* align = nullptr;
  const BeamTrace* trace = nullptr;
};

// ccx_whisper_align's hook in dec_step: the cross-attention probabilities of layer l's selected heads for the step's query rows
int align_scores_hook(ccx_whisper* w, const AlignPass& a, int l, const float* dq, int B, hipStream_t stream) {
  if (a.count[l] == 0) return CCX_OK;
  AlignScoresParams p{dq, w->dec[l].crossK, w->d.n_text_head, w->Spad, a.heads + a.first[l], a.hsel + a.first[l], a.count[l], a.n_keys,
                      w->al_P, a.Hsel, a.T, a.Mmax, a.t};
  return ccx_launch_align_scores(w->ctx, p, B, stream);
}

// what the select kernel and the beam kernels share; the row-addressed fields are the caller's
void fill_select_params(const ccx_whisper* w, const StepPlan& p, const StepIo& io, DecSelectParams& sp) {
  sp.logits = io.logits; sp.ld_logits = io.ld; sp.n_vocab = w->V4; sp.pos = w->pos + p.b0; sp.sample_len = p.sample_len; sp.n_done = io.n_done;
  sp.suppress_mask = p.opt_mask ? w->opt_mask : w->suppress_mask; sp.eot = w->rules.eot; sp.blank = w->rules.blank;
  sp.no_speech = w->rules.no_speech; sp.timestamp_begin = w->rules.timestamp_begin;
  sp.max_initial_ts = p.max_init_ts;
  sp.no_rules = p.no_ts; sp.suppress_blank = p.sup_blank;
  sp.tok_emb = w->tok_emb_f32; sp.pos_emb = w->dec_pos; sp.D = w->d.n_text_state;
}

// Tail of a step for the sequences [b0, b0 + B): logits of the final-LayerNorm rows (w->dxn) against the tied embedding, then
// the select kernel (filters, argmax / sampling, state machine, next step's embedding).
int dec_head(ccx_whisper* w, const StepPlan& p, const StepIo& io) {
  ccx_ctx* ctx = w->ctx;
  const ccx_whisper_dims& d = w->d;
  const int D = d.n_text_state, b0 = p.b0, B = p.B;
  const long ro = b0;
  {
    // logits against the tied embedding through the tiled GEMM (one summation order for every batch size; 284 -> 282 ms
    // for 192 sequences x 65 steps against the skinny kernel, no change at 8 sequences)
    GemmParams gp;
    memset(&gp, 0, sizeof(gp));
    gp.A = w->dxn + ro * D; gp.lda = D; gp.W = w->tok_emb_rm; gp.ldw = D; gp.M = B; gp.N = d.n_vocab; gp.K = D; gp.out = io.logits; gp.ldo = io.ld;
    CCX_TRY(ccx_launch_gemm(ctx, EPI_F32, gp, io.stream));
  }
  if (p.select && p.bias_on) {
    // the sequence bias edits the logit rows in place before the history rules and every filter (beam rows: the history that follows
    // the hypothesis)
    DecBiasParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.logits = io.logits; bp.ld = io.ld; bp.state = w->state + b0; bp.gen = w->gen + ro * p.sample_len; bp.sample_len = p.sample_len;
    bp.text_end = w->rules.eot; bp.tab = w->bias_tab;
    CCX_TRY(ccx_launch_dec_bias(ctx, bp, B, io.stream));
  }
  if (p.select && (p.hist_ngram || p.hist_pen_bits)) {
    // the history rules edit the logit rows in place before any filter reads them (beam rows: the history that follows the hypothesis)
    DecHistoryParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.logits = io.logits; hp.ld = io.ld; hp.state = w->state + b0; hp.gen = w->gen + ro * p.sample_len; hp.sample_len = p.sample_len;
    hp.text_end = w->rules.eot; hp.ngram = p.hist_ngram;
    hp.penalty = 1.f;
    if (p.hist_pen_bits) memcpy(&hp.penalty, &p.hist_pen_bits, 4);
    CCX_TRY(ccx_launch_dec_history(ctx, hp, B, io.stream));
  }
  if (p.select && p.beam_size > 0) {
    // beam search: the row's top beam + 1 proposals, then one block per window ranks, walks and rewrites its rows in place
    DecBeamParams bp;
    memset(&bp, 0, sizeof(bp));
    CCX_REQUIRE(ctx, b0 == 0 && B % p.beam_size == 0, "dec_head: a beam decode runs in one lane of whole windows");
    fill_select_params(w, p, io, bp.sel);
    bp.sel.state = w->state; bp.sel.cur_tok = w->cur_tok; bp.sel.gen = w->gen; bp.sel.x = w->dx;
    bp.beam = p.beam_size; bp.max_cand = p.beam_maxc; bp.cand_id = w->beam_cand_id; bp.cand_lp = w->beam_cand_lp;
    bp.ind = w->beam_ind; bp.ind_ld = d.n_text_ctx; bp.row0 = 0;
    bp.fin_tok = w->beam_fin_tok; bp.fin_score = w->beam_fin_score; bp.fin_n = w->beam_fin_n; bp.fin_count = w->beam_fin_count;
    if (const BeamTrace* t = io.trace) {
      bp.tr_cand_id = t->cid; bp.tr_cand_lp = t->clp; bp.tr_tok = t->tok; bp.tr_parent = t->par; bp.tr_score = t->score; bp.tr_rows = B;
    }
    CCX_TRY(ccx_launch_dec_beam(ctx, bp, B / p.beam_size, io.stream));
  } else if (p.select) {
    DecSelectParams sp;
    memset(&sp, 0, sizeof(sp));
    fill_select_params(w, p, io, sp);
    sp.state = w->state + b0; sp.prompt = w->prompt + ro * p.max_prompt; sp.max_prompt = p.max_prompt;
    sp.cur_tok = w->cur_tok + b0; sp.gen = w->gen + ro * p.sample_len; sp.x = w->dx + ro * D;
    sp.sample_cfg = w->sample_cfg; sp.row0 = b0; sp.sample = p.sampling ? 1 : 0;
    sp.trunc = p.trunc_on;
    if (p.logp) {
      sp.tok_logprob = w->tok_lp + ro * p.sample_len; sp.top_n = p.logp - 1;
      sp.top_id = w->top_id + ro * p.sample_len * CCX_LOGPROB_MAX_TOP; sp.top_lp = w->top_lp + ro * p.sample_len * CCX_LOGPROB_MAX_TOP;
    }
    sp.stream_id = p.sid_on ? w->row_sid + b0 : nullptr;
    CCX_TRY(ccx_launch_dec_select(ctx, sp, B, io.stream));
  }
  return CCX_OK;
}

// One decoder step for the B sequences [b0, b0 + B) of the plan on io.stream (a "lane": every per-sequence buffer is
// addressed through its row offset, so disjoint lanes can step concurrently on different streams).
// The residual stream ping-pongs between dx and dx2: out-proj / cross-out / FFN2 only write split-K partial slabs (pend) and the
// next LayerNorm folds them in (decoder.hip).
// plan.prefill_rows = P > 0: the PROMPT PREFILL pass instead of a step -- B sequences x P prompt positions as B * P rows of the pf_*
// buffers (row = sequence * P + position), self-KV written at every position, cross attention with all rows of a sequence
// sharing its K/V, no logits / select (the caller takes the last prompt row of every sequence).
// Reads the plan, io and instance-constant members of w only (StepPlan's invariant).
int dec_step(ccx_whisper* w, const StepPlan& p, const StepIo& io) {
  ccx_ctx* ctx = w->ctx;
  const ccx_whisper_dims& d = w->d;
  const int D = d.n_text_state, F = 4 * D, H = d.n_text_head, Tc = d.n_text_ctx;
  const float scale_log2e = 0.125f * 1.4426950408889634f;
  const int b0 = p.b0, nseq = p.B, prefill_rows = p.prefill_rows, lane_idx = p.lane_idx;
  const bool pre = prefill_rows > 0, map_on = p.map_on != 0, xs_active = p.xs_active != 0;
  const int B = pre ? nseq * prefill_rows : nseq;      // rows the chain works on
  const int ns = cross_split(nseq, H, p.cross_stream != 0);
  const long pstride = (long)B * D;
  const long ro = b0;
  hipStream_t stream = io.stream;
  float* cur = pre ? w->pf_x : w->dx + ro * D;     // stream (minus the pending partials); the step's embedding is in dx
  float* other = pre ? w->pf_x2 : w->dx2 + ro * D;
  float* pend = pre ? w->pf_pend : w->pend + 4 * ro * D;
  float* dq = pre ? w->pf_q : w->dq + ro * D;
  bf16_t* dxn = pre ? w->pf_xn : w->dxn + ro * D;
  bf16_t* dattn = pre ? w->pf_attn : w->dattn + ro * D;
  bf16_t* dffn = pre ? w->pf_ffn : w->dffn + ro * F;
  float* part_o = w->part_o + ro * H * ccx_whisper::kCrossSplitMax * 64;
  float* part_ml = w->part_ml + ro * H * ccx_whisper::kCrossSplitMax * 2;
  int* pos = pre ? w->pf_pos : w->pos + b0;
  const int* row_seq = pre ? w->pf_seq : nullptr;
  // mapped decode: the cross attention of row r reads window win[r] (prefill: the composed table), counted from window 0 -- the lane's
  // offset is in the map, not in the K/V base
  const int* win = !map_on ? nullptr : (pre ? w->pf_win : w->row_win + b0);
  const long cross_off = map_on ? 0 : ro * H * w->Spad * 64, self_off = ro * H * Tc * 64;
  auto stamp = [&](int tag, int level) {
    if (level <= p.stamp_level)
      hipLaunchKernelGGL(dec_stamp_kernel, dim3(1), dim3(1), 0, stream, w->stamps + (size_t)lane_idx * ccx_whisper::kStampCap,
                         w->stamp_count + lane_idx, ccx_whisper::kStampCap, tag);
  };
  // The > 16-row chain hands dxn (LayerNorm rows -> q|k|v, fc1, the query of its own launch) and dffn (fc1's GELU rows -> fc2) from
  // kernel to kernel as fragment images: the consumers' column blocks (72 - 96 per launch) each re-read all rows out of L2, and a CU
  // pulls a 1 KB-contiguous wave load about three times as fast as 16 rows x 64 B (profiles/dec_full_lines_experiment.txt).  Whole
  // 16-row tiles only, so that a lane's image ends where the next lane's begins; the rows the head and the prefill gather read (the
  // final LayerNorm) stay row-major.
  const int packed = ccx_dec_rows_as_image(p.packed_act, B);
  // ... and, under a switch of their own, the rest of its bf16 rows: dattn (self attention -> Wo, value projection -> Wco: 24 column
  // blocks each) and xb (Wo's resolve epilogue -> the LayerNorm-free query, 12 heads' blocks per row tile).  A decode step's lanes only:
  // the prefill, mapped rows (their launches stay what they were), the beam's indirect self attention and every K/V-cache path keep
  // row-major rows.
  const int packed_mid = (ccx_dec_rows_as_image(p.packed_mid, B) && !pre && !map_on && p.beam_size == 0 && xs_active && p.lnfree) ? 1 : 0;
  int pend_n = 0;
  auto ln_linear = [&](int epi, const bf16_t* W, const float* bias, int N, const float* g, const float* bta, void* out, long ldo,
                       DecLinearParams* extra) -> int {
    DecLinearParams lp;
    if (extra) lp = *extra; else memset(&lp, 0, sizeof(lp));
    lp.M = B; lp.N = N; lp.K = D; lp.W = W; lp.ldw = D; lp.bias = bias; lp.out = out; lp.ldo = ldo;
    int rc;
    if (B > 16) {
      // many sequences: normalise ONCE in a stand-alone kernel instead of redundantly in every weight-panel block
      rc = ccx_launch_dec_resolve_ln(ctx, cur, pend, pend_n, pstride, g, bta, dxn, pend_n > 0 ? other : nullptr, B, D, 1e-5f, stream,
                                     lp.ln_mean_out, packed);
      if (rc) return rc;
      lp.ln_mean_out = nullptr;
      lp.act = dxn; lp.lda = D; lp.act_packed = packed;
      rc = ccx_launch_dec_linear(ctx, ACT_BF16, epi, lp, stream);
    } else {
      lp.x = cur; lp.pend = pend; lp.pend_n = pend_n; lp.pend_stride = pstride; lp.x_out = pend_n > 0 ? other : nullptr;
      lp.ln_g = g; lp.ln_b = bta; lp.eps = 1e-5f;
      rc = ccx_launch_dec_linear(ctx, ACT_LN, epi, lp, stream);
    }
    if (rc) return rc;
    if (pend_n > 0) { float* t = cur; cur = other; other = t; pend_n = 0; }
    return CCX_OK;
  };
  auto partial_linear = [&](int act, const bf16_t* W, const float* bias, int K, const bf16_t* a, int a_packed = 0) -> int {
    DecLinearParams lp;
    memset(&lp, 0, sizeof(lp));
    lp.M = B; lp.N = D; lp.K = K; lp.W = W; lp.ldw = K; lp.bias = bias; lp.act = a; lp.lda = K; lp.act_packed = a_packed;
    lp.part_o = part_o; lp.part_ml = part_ml; lp.nsplit = ns;
    lp.out = pend; lp.ldo = D; lp.pend_stride = pstride;
    int rc = ccx_launch_dec_linear(ctx, act, DEPI_PARTIAL, lp, stream);
    if (rc) return rc;
    pend_n = ccx_dec_linear_ksplit(K, DEPI_PARTIAL);
    return CCX_OK;
  };
  // The cross-attention form is decided once for the step:
  //  * X-stream (xs_active: decodes of more than 80 sequences): one pass over the encoder output serves all heads (cross_x.hip).
  //    Its query is LayerNorm-free by default: the self-attention output projection resolves the residual in place and leaves a bf16
  //    copy of the rows plus their statistics (DEPI_RESOLVE), and the query applies its LayerNorm algebraically (gamma folded into
  //    Wcq_g) instead of a twelve-fold resolve + LayerNorm inside the expansion kernel: -1.0 ... -1.2 % per decode step.
  //    CCX_DEC_LNFREE=0: round 3's query -- resolve + LayerNorm inside the expansion kernel (CCX_XS_FUSE_Q=0: as a launch of its own).
  //  * <= 16 rows, d_model 768 (the reference's one-window-per-call pattern): the query projection LN(x) Wcq^T runs INSIDE the
  //    cross-attention blocks (ccx_launch_dec_cross_fused_q: one launch fewer per layer on a chain that is latency-bound launch by
  //    launch; q is bit-identical to the two-launch path).  CCX_FUSE_CROSS_Q=0 restores the two launches.
  //  * prefill: all prompt rows of a sequence share its K/V.
  //  * otherwise the K/V caches: > 16 rows lean streaming (split-KV partials + combine in ccx_whisper_decoder_logits), <= 16 rows
  //    split-KV partials combined by the out projection.
  const bool lnfree = xs_active && p.lnfree;
  const bool xs_fused = xs_active && !lnfree && p.xs_fuse_q;
  // (a mapped decode bypasses the fused query for the two launches it replaces: q is bit-identical, and the fused kernel's address
  //  arithmetic -- block-uniform bases in SGPR pairs under a 168-register cap -- stays what it is)
  const bool fuse_q = !xs_active && p.fuse_cross_q && !pre && B <= 16 && D == 768 && !map_on;
  const bool q_launch = !fuse_q && !lnfree && !xs_fused;    // the query projection as a launch of its own
  // LayerNorm-free query: the resolved rows and their tile statistics (X-stream instances only)
  bf16_t* xb = !lnfree ? nullptr : (pre ? w->pf_xb : w->dxb + ro * D);
  float2* st2 = !lnfree ? nullptr : (pre ? w->pf_st2 : w->dst2 + ro * (D / 16));
  float* shift = !lnfree ? nullptr : (pre ? w->pf_shift : w->dshift + ro);
  for (int l = 0; l < d.n_text_layer; l++) {
    const DecLayer& L = w->dec[l];
    // LN + QKV, k/v appended to the self cache at pos[b]
    {
      DecLinearParams ex;
      memset(&ex, 0, sizeof(ex));
      ex.cache_k = L.selfK + self_off; ex.cache_v = L.selfV + self_off; ex.cache_T = Tc; ex.pos = pos; ex.row_seq = row_seq;
      ex.ln_mean_out = shift;                      // LayerNorm-free query: the rows' attn_ln means centre their bf16 copies
      CCX_TRY(ln_linear(DEPI_SELF_QKV, L.Wqkv, L.bqkv, 3 * D, L.ln1_g, L.ln1_b, dq, D, &ex));
      stamp(16, 2);
    }
    DecAttnParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.q = dq; ap.k = L.selfK + self_off; ap.v = L.selfV + self_off; ap.H = H; ap.kv_T = Tc; ap.pos = pos; ap.scale_log2e = scale_log2e;
    ap.out_bf16 = dattn; ap.row_seq = row_seq;
    // beam search: a step's keys come through the cache indirection (the prefill writes and reads every row's own slot)
    if (p.beam_size > 0 && !pre) { ap.ind = w->beam_ind; ap.ind_ld = Tc; }
    ap.out_packed = packed_mid;
    CCX_TRY(ccx_launch_dec_attention(ctx, ap, B, 1, true, stream));
    stamp(17, 2);
    if (lnfree) {
      DecLinearParams lp;
      memset(&lp, 0, sizeof(lp));
      lp.M = B; lp.N = D; lp.K = D; lp.W = L.Wo; lp.ldw = D; lp.bias = L.bo; lp.act = dattn; lp.lda = D;
      lp.act_packed = packed_mid; lp.out_packed = packed_mid;     // dattn in, xb out
      lp.xres = cur; lp.xb = xb; lp.st_out = st2; lp.shift = shift; lp.shift_c = L.bo_mean;
      CCX_TRY(ccx_launch_dec_linear(ctx, ACT_BF16, DEPI_RESOLVE, lp, stream));
    } else {
      CCX_TRY(partial_linear(ACT_BF16, L.Wo, L.bo, D, dattn));
    }
    stamp(18, 2);
    // cross attention
    if (q_launch) CCX_TRY(ln_linear(DEPI_F32, L.Wcq, L.bcq, D, L.lnc_g, L.lnc_b, dq, D, nullptr));
    if (io.align) CCX_TRY(align_scores_hook(w, *io.align, l, dq, B, stream));   // ccx_whisper_align only: the step's row of P
    stamp(1, 1);
    if (l == 0 && io.stagger) CCX_HIP(ctx, hipEventRecord(io.stagger, stream));
    if (xs_active) {
      XsParams xp;
      memset(&xp, 0, sizeof(xp));
      if (lnfree) {
        xp.xb = xb; xp.xb_packed = packed_mid; xp.ln_stats = st2; xp.ln_s = L.scq; xp.Wq = L.Wcq_g; xp.bq = L.ccq; xp.eps = 1e-5f;
      } else if (xs_fused) {
        xp.x = cur; xp.pend = pend; xp.pend_n = pend_n; xp.pend_stride = pstride; xp.x_out = pend_n > 0 ? other : nullptr;
        xp.ln_g = L.lnc_g; xp.ln_b = L.lnc_b; xp.eps = 1e-5f; xp.Wq = L.Wcq_plain; xp.bq = L.bcq;
      }
      xp.q = dq; xp.WkT = L.WckT; xp.xq = pre ? w->pf_xq : w->xq + ro * H * D;
      xp.part_o = pre ? w->pf_xs_po : w->xs_po + ccx_xs_part_o_elems(ro, H, D);
      xp.part_ml = pre ? w->pf_xs_pml : w->xs_pml + ccx_xs_part_ml_elems(ro);
      xp.X = (pre || map_on) ? w->xa : w->xa + ro * (long)d.n_audio_ctx * D; xp.x_seq_stride = (long)d.n_audio_ctx * D;
      xp.row_seq = map_on ? win : row_seq;
      if (w->audio_ctx) xp.seq_S = (pre || map_on) ? w->xa_n : w->xa_n + ro;      // indexed as X is
      xp.Wv = L.Wcv_x; xp.bv = L.bckv + D; xp.out = dattn; xp.out_packed = packed_mid;
      xp.rows = B; xp.H = H; xp.S = d.n_audio_ctx; xp.D = D; xp.scale_log2e = scale_log2e;
      xp.lds_pad = (p.cross_lds_pad > 0 && !pre) ? 65536 : 0;
      xp.rows_per_seq = pre ? prefill_rows : 0;
      xp.full_lines = p.xs_full_lines;
      if (p.xs_fp8) { xp.X8 = (pre || map_on) ? w->xa8 : w->xa8 + ro * w->xa8_stride; xp.x8_seq_stride = w->xa8_stride; }
      CCX_TRY(ccx_launch_xs_cross_attention(ctx, xp, stream));
      if (xs_fused && pend_n > 0) { float* t = cur; cur = other; other = t; pend_n = 0; }
      stamp(2, 1);
      CCX_TRY(partial_linear(ACT_BF16, L.Wco, L.bco, D, dattn, packed_mid));
      stamp(19, 2);
    } else {
      memset(&ap, 0, sizeof(ap));
      ap.q = dq; ap.k = L.crossK + cross_off; ap.v = L.crossV + cross_off; ap.H = H; ap.kv_T = w->Spad; ap.pos = nullptr; ap.T = d.n_audio_ctx;
      ap.scale_log2e = scale_log2e; ap.part_o = part_o; ap.part_ml = part_ml; ap.out_bf16 = dattn;
      ap.lds_pad = p.cross_lds_pad;
      ap.stream_mode = (p.cross_stream && B > 16) ? 1 : 0;
      ap.row_seq = win; ap.kv_map = map_on ? 1 : 0;
      if (fuse_q) {
        ap.qx = cur; ap.q_pend = pend; ap.q_pend_n = pend_n; ap.q_pend_stride = pstride; ap.q_x_out = pend_n > 0 ? other : nullptr;
        ap.q_ln_g = L.lnc_g; ap.q_ln_b = L.lnc_b; ap.q_eps = 1e-5f; ap.q_W = L.Wcq; ap.q_bias = L.bcq; ap.q_K = D;
        CCX_TRY(ccx_launch_dec_cross_fused_q(ctx, ap, B, ns, stream));
        if (pend_n > 0) { float* t = cur; cur = other; other = t; pend_n = 0; }
        CCX_TRY(partial_linear(ACT_COMBINE, L.Wco, L.bco, D, nullptr));
      } else if (pre) {
        // two prompt rows and more per sequence share its K/V; a one-row pass runs as a decode step would
        if (!map_on) ap.row_seq = prefill_rows > 1 ? row_seq : nullptr;
        ap.rows_per_seq = prefill_rows > 1 ? prefill_rows : 0;
        ap.lds_pad = 0; ap.stream_mode = 1;
        CCX_TRY(ccx_launch_dec_attention(ctx, ap, nseq, 1, true, stream));
        CCX_TRY(partial_linear(ACT_BF16, L.Wco, L.bco, D, dattn));
      } else if (B > 16) {
        CCX_TRY(ccx_launch_dec_attention(ctx, ap, B, ns, ns == 1, stream));
        stamp(2, 1);
        if (ns > 1) CCX_TRY(ccx_launch_dec_combine(ctx, part_o, part_ml, ns, dattn, B, H, stream));
        CCX_TRY(partial_linear(ACT_BF16, L.Wco, L.bco, D, dattn));
        stamp(19, 2);
      } else {
        CCX_TRY(ccx_launch_dec_attention(ctx, ap, B, ns, false, stream));
        CCX_TRY(partial_linear(ACT_COMBINE, L.Wco, L.bco, D, nullptr));
      }
    }
    // MLP.  (fc1 through the tiled GEMM from 256 rows on, 653.1 -> 647.6 ms per pipeline step, was removed: the GEMM sums K in
    // another order, so a sequence's log-probabilities would depend on its lane's row count -- DESIGN.md)
    {
      DecLinearParams ex;
      memset(&ex, 0, sizeof(ex));
      ex.out_packed = packed;
      CCX_TRY(ln_linear(DEPI_BF16_GELU, L.W1, L.b1, F, L.ln2_g, L.ln2_b, dffn, F, &ex));
    }
    stamp(20, 2);
    CCX_TRY(partial_linear(ACT_BF16, L.W2, L.b2, F, dffn, packed));
    stamp(21, 2);
  }
  // resolve the last partials + final LN, then logits against the tied embedding
  CCX_TRY(ccx_launch_dec_resolve_ln(ctx, cur, pend, pend_n, pstride, w->lnd_g, w->lnd_b, dxn, nullptr, B, D, 1e-5f, stream));
  if (pre) return CCX_OK;         // the caller gathers the last prompt row of every sequence out of pf_xn
  CCX_TRY(dec_head(w, p, io));
  stamp(3, 1);       // end of the step
  return CCX_OK;
}

// `prefilled`: the prompts go through the prefill pass, so every sequence starts at its LAST prompt position (the state machine's
// sampling phase) and the first embedding comes from the prefill, not from here.
int upload_decode_state(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int B,
                        float temperature, uint64_t seed, hipStream_t stream, bool prefilled = false) {
  std::vector<DecSeqState> st(B);
  std::vector<int> tok(B), ps(B, 0);
  for (int b = 0; b < B; b++) {
    memset(&st[b], 0, sizeof(DecSeqState));
    st[b].prompt_len = prompt_lens[b];
    st[b].last_tok = -1; st[b].pen_tok = -1; st[b].last_ts_tok = -1;
    tok[b] = prompt_ids[(size_t)b * max_prompt];
    if (prefilled) {
      st[b].pos = prompt_lens[b] - 1;
      ps[b] = prompt_lens[b] - 1;
      tok[b] = prompt_ids[(size_t)b * max_prompt + prompt_lens[b] - 1];
    }
  }
  CCX_HIP(w->ctx, hipMemcpyAsync(w->state, st.data(), B * sizeof(DecSeqState), hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipMemcpyAsync(w->cur_tok, tok.data(), B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipMemcpyAsync(w->pos, ps.data(), B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipMemcpyAsync(w->prompt, prompt_ids, (size_t)B * max_prompt * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(w->ctx, hipMemsetAsync(w->n_done, 0, ccx_whisper::kMaxLanes * 4, stream));
  unsigned cfg[8];
  ccx_fill_sample_cfg(cfg, temperature, seed, w->trunc);
  CCX_HIP(w->ctx, hipMemcpyAsync(w->sample_cfg, cfg, sizeof(cfg), hipMemcpyHostToDevice, stream));
  // embedding of the first token; later steps get theirs from the select kernel
  if (!prefilled) CCX_TRY(ccx_launch_dec_embed(w->ctx, w->tok_emb_f32, w->dec_pos, w->cur_tok, w->pos, w->dx, B, w->d.n_text_state, stream));
  CCX_HIP(w->ctx, hipStreamSynchronize(stream));  // host vectors go out of scope
  return CCX_OK;
}

// Prompt prefill (openai-whisper's first forward over all initial tokens, decoding.py::_main_loop): every prompt position of every
// sequence through the layer chain in passes of up to kPrefillMax positions -- rows = sequence * Pc + (position - first position of
// the pass); a pass sees the self-K/V of the earlier passes in the caches, so a long prompt (the reference feeds the previous
// segment's transcript as `initial_prompt`, up to 223 tokens: back/api.py:1424-1426) costs one pass per 16 tokens instead of one
// decode step per token.  Positions past a shorter prompt are dead rows (their K/V land beyond the prompt and are overwritten by the
// tokens decoded there later).  Leaves the self-KV caches filled and the final-LayerNorm row of every sequence's last prompt
// position in w->dxn -- and, for instances whose no-speech probability is read at the SOT position (ns_at_sot), the row of prompt
// position prompt_len - 1 - sot_tail in w->tp_xn, gathered in whichever pass holds it (it can be the pass before the last token's).
// `plan`: the decode's plan over all its rows; `win_host`: the host copy of its row -> window map (plan.map_on), else null.
int run_prefill(ccx_whisper* w, const StepPlan& plan, const int32_t* win_host, const int32_t* prompt_ids, const int32_t* prompt_lens, int P,
                hipStream_t stream) {
  ccx_ctx* ctx = w->ctx;
  const int D = w->d.n_text_state, C = ccx_whisper::kPrefillMax, B = plan.B, max_prompt = plan.max_prompt;
  StepPlan pass = plan;
  pass.select = 0;
  StepIo io;
  io.stream = stream;
  for (int t0 = 0; t0 < P; t0 += C) {
    const int Pc = P - t0 < C ? P - t0 : C, R = B * Pc;
    std::vector<int> tok(R), ps(R), sq(R), last(B), sot_row(B);
    for (int b = 0; b < B; b++) {
      for (int t = 0; t < Pc; t++) {
        const int r = b * Pc + t, ta = t0 + t;
        tok[r] = ta < prompt_lens[b] ? prompt_ids[(size_t)b * max_prompt + ta] : w->rules.eot;
        ps[r] = ta; sq[r] = b;
      }
      const int tl = prompt_lens[b] - 1 - t0;        // the sequence's last prompt position, relative to this pass
      last[b] = (tl >= 0 && tl < Pc) ? b * Pc + tl : -1;
      const int ts = tl - w->sot_tail - w->prefix_len;   // ... and its <|startoftranscript|>
      sot_row[b] = (ts >= 0 && ts < Pc) ? b * Pc + ts : -1;
    }
    if (w->ns_at_sot()) CCX_HIP(ctx, hipMemcpyAsync(w->tp_idx, sot_row.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream));
    CCX_HIP(ctx, hipMemcpyAsync(w->pf_tok, tok.data(), (size_t)R * 4, hipMemcpyHostToDevice, stream));
    CCX_HIP(ctx, hipMemcpyAsync(w->pf_pos, ps.data(), (size_t)R * 4, hipMemcpyHostToDevice, stream));
    CCX_HIP(ctx, hipMemcpyAsync(w->pf_seq, sq.data(), (size_t)R * 4, hipMemcpyHostToDevice, stream));
    std::vector<int> wn(plan.map_on ? R : 0);   // mapped decode: the two maps composed, a prefill row's window is win[pf_seq[row]]
    if (plan.map_on) {
      for (int r = 0; r < R; r++) wn[r] = win_host[sq[r]];
      CCX_HIP(ctx, hipMemcpyAsync(w->pf_win, wn.data(), (size_t)R * 4, hipMemcpyHostToDevice, stream));
    }
    CCX_HIP(ctx, hipMemcpyAsync(w->pf_last, last.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream));
    CCX_TRY(ccx_launch_dec_embed(ctx, w->tok_emb_f32, w->dec_pos, w->pf_tok, w->pf_pos, w->pf_x, R, D, stream));
    CCX_HIP(ctx, hipStreamSynchronize(stream));     // host tables go out of scope
    pass.prefill_rows = Pc;
    CCX_TRY(dec_step(w, pass, io));
    CCX_TRY(ccx_launch_dec_gather_rows(ctx, w->pf_xn, w->pf_last, w->dxn, B, D, stream));
    if (w->ns_at_sot()) CCX_TRY(ccx_launch_dec_gather_rows(ctx, w->pf_xn, w->tp_idx, w->tp_xn, B, D, stream));
  }
  return CCX_OK;
}

// scratch of the ranged softmax's users, on first use (sized from max_batch)
int ensure_token_probs_scratch(ccx_whisper* w) {
  if (w->tp_xn) return CCX_OK;
  const size_t B = (size_t)w->max_batch;
  CCX_TRY(w->store.alloc(&w->tp_idx, B, true));
  CCX_TRY(w->store.alloc(&w->tp_arg, B, true));
  CCX_TRY(w->store.alloc(&w->tp_prob, B, true));
  CCX_TRY(w->store.alloc(&w->tp_lang, B * ccx_whisper::kMaxLang, true));
  CCX_TRY(w->store.alloc(&w->tp_xn, B * w->d.n_text_state, true));
  return CCX_OK;
}

// logits of the B final-LayerNorm rows `xn` against the tied embedding into w->dlogits (dec_head's GEMM), then the softmax over the
// ids [lo, hi): argmax -> w->tp_arg, probability of `pick` -> w->tp_prob, the range's distribution -> probs (device, may be null)
int token_probs_of_rows(ccx_whisper* w, const bf16_t* xn, int B, int lo, int hi, int pick, float* probs, hipStream_t stream) {
  const int D = w->d.n_text_state;
  GemmParams gp;
  memset(&gp, 0, sizeof(gp));
  gp.A = xn; gp.lda = D; gp.W = w->tok_emb_rm; gp.ldw = D; gp.M = B; gp.N = w->d.n_vocab; gp.K = D; gp.out = w->dlogits; gp.ldo = w->Vpad;
  CCX_TRY(ccx_launch_gemm(w->ctx, EPI_F32, gp, stream));
  DecTokenProbsParams tp;
  memset(&tp, 0, sizeof(tp));
  tp.logits = w->dlogits; tp.ld = w->Vpad; tp.lo = lo; tp.hi = hi; tp.pick = pick;
  tp.argmax = w->tp_arg; tp.pick_prob = w->tp_prob; tp.probs = probs;
  return ccx_launch_dec_token_probs(w->ctx, tp, B, stream);
}

}  // namespace

extern "C" {

int ccx_whisper_decoder_logits(ccx_whisper* w, const int32_t* tokens, int B, int T, float* logits_dev, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->finalized && w->rules_set, "whisper: not finalized or rules not set");
  CCX_REQUIRE(ctx, tokens && logits_dev && B >= 1 && B <= w->max_batch && T >= 1 && T <= w->d.n_text_ctx, "decoder_logits: bad arguments");
  for (long i = 0; i < (long)B * T; i++)
    CCX_REQUIRE(ctx, tokens[i] >= 0 && tokens[i] < w->d.n_vocab, "decoder_logits: token id %d out of range", tokens[i]);
  std::vector<int32_t> lens(B, T + 1);  // never leaves the prompt phase: every step feeds tokens[b][pos]
  // prompt buffer rows are `T` wide here
  StepPlan plan = single_lane_plan(w, B, T);
  plan.cross_stream = 0;
  CCX_TRY(select_cross_path(w, plan, stream));
  CCX_TRY(upload_decode_state(w, tokens, lens.data(), T, B, 0.f, 0, stream));
  const long V = w->d.n_vocab;
  StepIo io;
  io.logits = w->dlogits; io.ld = w->Vpad; io.n_done = w->n_done; io.stream = stream;
  for (int t = 0; t < T; t++) {
    // the select kernel (prompt phase) advances cur_tok/pos; on the last step it would read prompt[T] -> skip it.
    // The logits GEMM stores whole 16-column groups, so it writes the padded workspace rows (ld = Vpad) and the n_vocab valid
    // columns are copied out: writing [B, T, V] in place would spill V % 16 columns into the next row / past the tensor.
    plan.select = t + 1 < T;
    CCX_TRY(dec_step(w, plan, io));
    CCX_HIP(ctx, hipMemcpy2DAsync(logits_dev + (long)t * V, (size_t)T * V * 4, w->dlogits, (size_t)w->Vpad * 4, (size_t)V * 4, B,
                                  hipMemcpyDeviceToDevice, stream));
  }
  return CCX_OK;
}

int ccx_whisper_align(ccx_whisper* w, const int32_t* tokens, const int32_t* lens, int max_len, int B, const int32_t* n_frames,
                      const int32_t* heads, int n_heads, int row0, float* probs_out_dev, float* matrix_out_dev, int32_t* jump_frame_out,
                      void* stream_) {
  return ccx_whisper_align_probs(w, tokens, lens, max_len, B, n_frames, heads, n_heads, row0, probs_out_dev, matrix_out_dev, jump_frame_out, 0,
                                 nullptr, stream_);
}

// The messages keep the name ccx_whisper_align: that is the pass, with or without the token probabilities.
int ccx_whisper_align_probs(ccx_whisper* w, const int32_t* tokens, const int32_t* lens, int max_len, int B, const int32_t* n_frames,
                            const int32_t* heads, int n_heads, int row0, float* probs_out_dev, float* matrix_out_dev,
                            int32_t* jump_frame_out, int prob_hi, float* token_prob_out, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  ccx_ctx* ctx = w->ctx;
  const ccx_whisper_dims& d = w->d;
  CCX_REQUIRE(ctx, w->finalized && w->rules_set, "ccx_whisper_align: not finalized or rules not set");
  CCX_REQUIRE(ctx, tokens && lens && n_frames && heads && jump_frame_out, "ccx_whisper_align: tokens, lens, n_frames, heads or jump_frame_out is NULL");
  CCX_REQUIRE(ctx, B >= 1 && B <= w->max_batch, "ccx_whisper_align: B = %d out of range [1, max_batch = %d]", B, w->max_batch);
  CCX_REQUIRE(ctx, B <= w->kv_cap, "ccx_whisper_align: B = %d, the cross-attention K / V caches hold %d sequences", B, w->kv_cap);
  CCX_REQUIRE(ctx, max_len >= 2 && max_len <= d.n_text_ctx && max_len <= CCX_ALIGN_MAX_TOK, "ccx_whisper_align: max_len = %d out of range [2, %d]", max_len,
              d.n_text_ctx < CCX_ALIGN_MAX_TOK ? d.n_text_ctx : CCX_ALIGN_MAX_TOK);
  CCX_REQUIRE(ctx, d.n_audio_ctx <= CCX_ALIGN_MAX_FRAMES, "ccx_whisper_align: n_audio_ctx = %d, the kernels hold %d frames", d.n_audio_ctx, CCX_ALIGN_MAX_FRAMES);
  CCX_REQUIRE(ctx, n_heads >= 1 && n_heads <= CCX_ALIGN_MAX_HEADS, "ccx_whisper_align: n_heads = %d out of range [1, %d]", n_heads, CCX_ALIGN_MAX_HEADS);
  CCX_REQUIRE(ctx, row0 >= 0, "ccx_whisper_align: row0 = %d is negative", row0);
  if (token_prob_out)
    CCX_REQUIRE(ctx, prob_hi >= 1 && prob_hi <= d.n_vocab, "ccx_whisper_align_probs: prob_hi = %d out of range [1, n_vocab = %d]", prob_hi, d.n_vocab);
  const int Mmax = d.n_audio_ctx, T = max_len, L = d.n_text_layer;
  std::vector<int> keys(B), r1(B), nrows(B);
  std::vector<int32_t> padded((size_t)B * T, w->rules.eot);
  for (int b = 0; b < B; b++) {
    CCX_REQUIRE(ctx, lens[b] >= row0 + 2 && lens[b] <= max_len, "ccx_whisper_align: lens[%d] = %d out of range [row0 + 2 = %d, max_len = %d]", b, lens[b], row0 + 2,
                max_len);
    CCX_REQUIRE(ctx, n_frames[b] >= 2 && n_frames[b] <= 2 * Mmax, "ccx_whisper_align: n_frames[%d] = %d out of range [2, %d]", b, n_frames[b], 2 * Mmax);
    keys[b] = n_frames[b] / 2; nrows[b] = lens[b]; r1[b] = lens[b] - 1;
    if (w->audio_ctx)
      CCX_REQUIRE(ctx, keys[b] <= w->enc_ctx[b], "ccx_whisper_align: n_frames[%d] = %d needs %d positions, window %d was encoded with an audio context of %d", b,
                  n_frames[b], keys[b], b, w->enc_ctx[b]);
    for (int t = 0; t < lens[b]; t++) {
      const int32_t tok = tokens[(size_t)b * max_len + t];
      CCX_REQUIRE(ctx, tok >= 0 && tok < d.n_vocab, "ccx_whisper_align: tokens[%d][%d] = %d out of range [0, n_vocab = %d)", b, t, tok, d.n_vocab);
      padded[(size_t)b * T + t] = tok;
    }
  }
  // token probabilities: row t predicts tokens[b][t + 1]; the text tokens are rows row0 .. lens[b] - 3 (find_alignment's
  // logits[len(sot_sequence):, :eot] at the text tokens); -1 everywhere else, which the kernel skips
  std::vector<int32_t> picks;
  if (token_prob_out) {
    picks.assign((size_t)B * T, -1);
    for (int b = 0; b < B; b++)
      for (int t = row0; t <= lens[b] - 3; t++) {
        const int32_t tok = padded[(size_t)b * T + t + 1];
        CCX_REQUIRE(ctx, tok < prob_hi, "ccx_whisper_align_probs: tokens[%d][%d] = %d is a text token at or behind prob_hi = %d", b, t + 1, tok, prob_hi);
        picks[(size_t)b * T + t] = tok;
      }
  }
  // (layer, head) pairs -> per-layer ranges of the device tables; P's head axis keeps the caller's order
  AlignPass pass;
  pass.first.assign(L, 0); pass.count.assign(L, 0);
  std::vector<int> h_heads, h_hsel;
  for (int i = 0; i < n_heads; i++) {
    const int l = heads[2 * i], h = heads[2 * i + 1];
    CCX_REQUIRE(ctx, l >= 0 && l < L && h >= 0 && h < d.n_text_head, "ccx_whisper_align: heads[%d] = (layer %d, head %d) outside %d layers x %d heads", i, l, h, L,
                d.n_text_head);
    for (int j = 0; j < i; j++)
      CCX_REQUIRE(ctx, heads[2 * j] != l || heads[2 * j + 1] != h, "ccx_whisper_align: heads[%d] repeats heads[%d] = (layer %d, head %d)", i, j, l, h);
  }
  for (int l = 0; l < L; l++) {
    pass.first[l] = (int)h_heads.size();
    for (int i = 0; i < n_heads; i++)
      if (heads[2 * i] == l) { h_heads.push_back(heads[2 * i + 1]); h_hsel.push_back(i); }
    pass.count[l] = (int)h_heads.size() - pass.first[l];
  }
  // workspaces: on first use, sized from max_batch (and grown if a later call selects more heads or longer rows)
  const size_t seqs = (size_t)(w->max_batch < w->kv_cap ? w->max_batch : w->kv_cap);
  const size_t Tcap = (size_t)(d.n_text_ctx / 2 + 4 > T ? d.n_text_ctx / 2 + 4 : T);
  const size_t P_need = seqs * n_heads * Tcap * Mmax, A_need = seqs * Tcap * Mmax, tr_need = seqs * (Tcap + 1) * (Mmax + 1);
  const size_t path_cap = (size_t)T + Mmax;
  const size_t ints_need = 2 * (size_t)CCX_ALIGN_MAX_HEADS + seqs * (4 + 2 * (Tcap + Mmax) + Tcap);
  // P is the large one: seqs x n_heads x Tcap x n_audio_ctx x 4 bytes -- 0.79 GB for small.en's 72 default heads at max_batch 8, 7.9 GB
  // at the 80 sequences the K / V caches of a large instance hold (include/ccx.h).  A buffer that has to grow is freed first.
  auto grow = [&](void** buf, size_t* have, size_t need_bytes) -> int {
    if (*have >= need_bytes) return CCX_OK;
    if (*buf) { CCX_HIP(ctx, hipStreamSynchronize(stream)); CCX_HIP(ctx, hipFree(*buf)); *buf = nullptr; *have = 0; }
    CCX_HIP(ctx, hipMalloc(buf, need_bytes));
    *have = need_bytes;
    return CCX_OK;
  };
  CCX_TRY(grow((void**)&w->al_P, &w->al_P_elems, P_need * sizeof(float)));
  CCX_TRY(grow((void**)&w->al_A, &w->al_A_elems, A_need * sizeof(float)));
  CCX_TRY(grow((void**)&w->al_trace, &w->al_trace_bytes, tr_need));
  CCX_TRY(grow((void**)&w->al_ints, &w->al_ints_elems, ints_need * sizeof(int)));
  float* tprob = nullptr;
  if (token_prob_out) {
    CCX_TRY(grow((void**)&w->al_picks, &w->al_picks_bytes, 2 * seqs * Tcap * 4));
    tprob = (float*)(w->al_picks + seqs * Tcap);
    CCX_HIP(ctx, hipMemcpyAsync(w->al_picks, picks.data(), (size_t)B * T * 4, hipMemcpyHostToDevice, stream));
  }
  int* i_heads = w->al_ints;
  int* i_hsel = i_heads + CCX_ALIGN_MAX_HEADS;
  int* i_keys = i_hsel + CCX_ALIGN_MAX_HEADS;
  int* i_rows = i_keys + seqs;
  int* i_r1 = i_rows + seqs;
  int* i_len = i_r1 + seqs;
  int* i_text = i_len + seqs;
  int* i_time = i_text + seqs * (Tcap + Mmax);
  int* i_jump = i_time + seqs * (Tcap + Mmax);
  CCX_HIP(ctx, hipMemcpyAsync(i_heads, h_heads.data(), (size_t)n_heads * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(ctx, hipMemcpyAsync(i_hsel, h_hsel.data(), (size_t)n_heads * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(ctx, hipMemcpyAsync(i_keys, keys.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(ctx, hipMemcpyAsync(i_rows, nrows.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(ctx, hipMemcpyAsync(i_r1, r1.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream));
  CCX_HIP(ctx, hipMemsetAsync(w->al_A, 0, (size_t)B * T * Mmax * 4, stream));
  pass.heads = i_heads; pass.hsel = i_hsel; pass.n_keys = i_keys; pass.Hsel = n_heads; pass.T = T; pass.Mmax = Mmax;

  // the pass runs on the per-layer K / V form with the query projection as a launch of its own: every row's query is in dq
  StepPlan plan = single_lane_plan(w, B, T);
  plan.cross_stream = 0;
  plan.fuse_cross_q = 0;
  plan.xs_active = 0;       // whatever the size: no select_cross_path here
  // a reduced-audio-context instance: the rows' cross attention must stop at their window's count, which only the X-stream does -- with
  // the query still a launch of its own (dq is what the hook reads).  K is projected as always and read up to n_frames / 2 <= the count
  if (w->audio_ctx) { plan.xs_active = 1; plan.lnfree = 0; plan.xs_fuse_q = 0; }
  if (w->kv_ready < B) CCX_TRY(project_cross_kv(w, B, stream));
  std::vector<int32_t> plens(B, T + 1);    // never leaves the prompt phase: every step feeds tokens[b][pos]
  CCX_TRY(upload_decode_state(w, padded.data(), plens.data(), T, B, 0.f, 0, stream));
  StepIo io;
  io.logits = w->dlogits; io.ld = w->Vpad; io.n_done = w->n_done; io.stream = stream; io.align = &pass;
  for (int t = 0; t < T; t++) {
    pass.t = t;
    plan.select = t + 1 < T;
    CCX_TRY(dec_step(w, plan, io));
    if (token_prob_out && t >= row0 && t <= T - 3) {      // only reads the step's logits: column t of the two [B][T] tables
      DecPickProbsParams pp{w->dlogits, (long)w->Vpad, prob_hi, w->al_picks + t, (long)T, tprob + t, (long)T};
      CCX_TRY(ccx_launch_dec_pick_probs(ctx, pp, B, stream));
    }
  }
  AlignMatrixParams mp{w->al_P, w->al_A, n_heads, T, Mmax, i_rows, i_keys};
  CCX_TRY(ccx_launch_align_matrix(ctx, mp, B, stream));
  AlignDtwParams dp{w->al_A, T, Mmax, row0, i_r1, i_keys, w->al_trace, (long)((size_t)(T + 1) * (Mmax + 1)), i_text, i_time, (int)path_cap, i_len, i_jump};
  CCX_TRY(ccx_launch_align_dtw(ctx, dp, B, stream));
  if (probs_out_dev) CCX_HIP(ctx, hipMemcpyAsync(probs_out_dev, w->al_P, (size_t)B * n_heads * T * Mmax * 4, hipMemcpyDeviceToDevice, stream));
  if (matrix_out_dev) CCX_HIP(ctx, hipMemcpyAsync(matrix_out_dev, w->al_A, (size_t)B * T * Mmax * 4, hipMemcpyDeviceToDevice, stream));
  CCX_HIP(ctx, hipMemcpyAsync(jump_frame_out, i_jump, (size_t)B * T * 4, hipMemcpyDeviceToHost, stream));
  std::vector<float> tp_host;
  if (token_prob_out) {
    tp_host.resize((size_t)B * T);
    CCX_HIP(ctx, hipMemcpyAsync(tp_host.data(), tprob, (size_t)B * T * 4, hipMemcpyDeviceToHost, stream));
  }
  CCX_HIP(ctx, hipStreamSynchronize(stream));
  if (token_prob_out)
    for (int b = 0; b < B; b++)
      for (int i = 0; i < T; i++)     // row row0 + i holds text token i; skipped rows were never written
        token_prob_out[(size_t)b * T + i] = i < lens[b] - row0 - 2 ? tp_host[(size_t)b * T + row0 + i] : -1.f;
  return CCX_OK;
}

int ccx_whisper_last_cross_path(ccx_whisper* w) { return w ? w->last_cross_path : -1; }

int ccx_whisper_set_sot_tail(ccx_whisper* w, int n_tail) {
  if (!w) return CCX_ERR_ARG;
  // [sot, <|language|>, <|task|>, <|notimestamps|>] is the longest SOT sequence there is, and a multilingual vocabulary's
  const int max_tail = w->d.n_vocab >= 51865 ? 3 : 2;
  CCX_REQUIRE(w->ctx, n_tail >= 0 && n_tail <= max_tail, "ccx_whisper_set_sot_tail: n_tail = %d out of range [0, %d]", n_tail, max_tail);
  w->sot_tail = n_tail;     // read by the host side of a decode only: the captured step graphs do not depend on it
  return CCX_OK;
}

int ccx_whisper_set_prefix_len(ccx_whisper* w, int n_prefix) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, n_prefix >= 0 && n_prefix <= w->d.n_text_ctx / 2, "ccx_whisper_set_prefix_len: n_prefix = %d out of range [0, n_text_ctx / 2 = %d]",
              n_prefix, w->d.n_text_ctx / 2);
  w->prefix_len = n_prefix;  // host side only, as the SOT tail
  return CCX_OK;
}

int ccx_whisper_detect_language(ccx_whisper* w, int B, int lang_begin, int n_lang, int32_t* lang_token_out, float* probs_out, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->finalized && w->rules_set, "ccx_whisper_detect_language: not finalized or rules not set");
  CCX_REQUIRE(ctx, B >= 1 && B <= w->max_batch, "ccx_whisper_detect_language: B = %d out of range [1, max_batch = %d]", B, w->max_batch);
  CCX_REQUIRE(ctx, n_lang >= 1 && n_lang <= ccx_whisper::kMaxLang, "ccx_whisper_detect_language: n_lang = %d out of range [1, %d]", n_lang, ccx_whisper::kMaxLang);
  CCX_REQUIRE(ctx, lang_begin >= 0 && lang_begin + n_lang <= w->d.n_vocab, "ccx_whisper_detect_language: ids [%d, %d) outside the vocabulary of %d", lang_begin,
              lang_begin + n_lang, w->d.n_vocab);
  CCX_REQUIRE(ctx, lang_token_out != nullptr, "ccx_whisper_detect_language: lang_token_out is NULL");
  CCX_REQUIRE(ctx, w->rules.sot >= 0, "ccx_whisper_detect_language: rules.sot = %d is no token", w->rules.sot);
  CCX_TRY(own_stream_if_null(w, &stream));     // as ccx_whisper_decode
  CCX_TRY(ensure_token_probs_scratch(w));
  // one step over [sot] at position 0 for every window: the step kernels and the cross-attention path select_cross_path picks for
  // B rows, as ONE lane (a decode of 96 rows and more splits into lanes; a row's numbers do not depend on the split)
  StepPlan plan = single_lane_plan(w, B, 1);
  CCX_TRY(select_cross_path(w, plan, stream));
  const std::vector<int32_t> sot(B, w->rules.sot), one(B, 1);
  CCX_TRY(upload_decode_state(w, sot.data(), one.data(), 1, B, 0.f, 0, stream));
  w->last_cross_path = plan.xs_active ? 2 : (B > 16 ? 1 : 0);
  StepIo io;
  io.logits = w->dlogits; io.ld = w->Vpad; io.n_done = w->n_done; io.stream = stream;
  CCX_TRY(dec_step(w, plan, io));
  // dec_step left the logits of every row in w->dlogits: the softmax over the language tokens only (the GEMM is not repeated)
  DecTokenProbsParams tp;
  memset(&tp, 0, sizeof(tp));
  tp.logits = w->dlogits; tp.ld = w->Vpad; tp.lo = lang_begin; tp.hi = lang_begin + n_lang; tp.pick = lang_begin;
  tp.argmax = w->tp_arg; tp.pick_prob = w->tp_prob; tp.probs = w->tp_lang;
  CCX_TRY(ccx_launch_dec_token_probs(ctx, tp, B, stream));
  CCX_HIP(ctx, hipMemcpyAsync(lang_token_out, w->tp_arg, (size_t)B * 4, hipMemcpyDeviceToHost, stream));
  if (probs_out) CCX_HIP(ctx, hipMemcpyAsync(probs_out, w->tp_lang, (size_t)B * n_lang * 4, hipMemcpyDeviceToHost, stream));
  CCX_HIP(ctx, hipStreamSynchronize(stream));
  return CCX_OK;
}

int ccx_whisper_prepare_lanes(ccx_whisper* w, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  CCX_REQUIRE(w->ctx, w->finalized, "whisper: not finalized");
  hipStream_t stream = stream_ ? (hipStream_t)stream_ : w->own_stream;
  CCX_HIP(w->ctx, hipDeviceSynchronize());
  (void)lane_streams_for(w, stream);
  return CCX_OK;
}

int ccx_whisper_decode_greedy(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int B,
                              int sample_len, int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out,
                              float* no_speech_prob_out, void* stream_) {
  // (the log-probability setting is not this entry point's: off for the call, as it was left behind it)
  const int logp_n = w ? w->logp_n : -1;
  if (w) w->logp_n = -1;
  const int rc = ccx_whisper_decode(w, prompt_ids, prompt_lens, max_prompt, B, sample_len, 0.f, 0, tokens_out, n_tokens_out, sum_logprob_out,
                                    no_speech_prob_out, stream_);
  if (w) w->logp_n = logp_n;
  return rc;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// the decode driver behind ccx_whisper_decode, ccx_whisper_decode_rows and ccx_whisper_decode_beam: decode_impl and its phases
// ---------------------------------------------------------------------------------------------
namespace {

struct BeamCall {
  int G, beam, maxc;
  int32_t* n_hyp_out;
  const ccx_beam_trace* trace;
};

// what one beam decode owns: the staged cache indirection (until the state upload synchronises) and a traced call's device buffers
struct BeamWork {
  std::vector<unsigned short> ind_init;
  BeamTrace trace;
  ~BeamWork() { hipFree(trace.cid); hipFree(trace.clp); hipFree(trace.tok); hipFree(trace.par); hipFree(trace.score); }
};

// a lane: its plan (select = 1), its io (its own stream, logits rows, done counter) and the step graph it replays, if any
struct Lane { StepPlan plan; StepIo io; hipGraphExec_t exec; };
struct Lanes {
  Lane lane[ccx_whisper::kMaxLanes];
  int n = 0;
};

// (1) the arguments of a decode.  -> *max_pl: the longest prompt
int check_decode_args(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int B, int sample_len, float temperature,
                      const int32_t* tokens_out, int* max_pl) {
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, temperature >= 0.f && temperature == temperature, "decode: temperature must be >= 0");
  CCX_REQUIRE(ctx, w->finalized && w->rules_set, "whisper: not finalized or rules not set");
  CCX_REQUIRE(ctx, prompt_ids && prompt_lens && tokens_out && B >= 1 && B <= w->max_batch, "decode_greedy: bad arguments");
  CCX_REQUIRE(ctx, sample_len >= 1 && sample_len <= w->sample_cap && max_prompt >= 1 && max_prompt <= w->max_prompt_cap, "decode_greedy: sample_len/max_prompt out of range");
  *max_pl = 0;
  for (int b = 0; b < B; b++) {
    CCX_REQUIRE(ctx, prompt_lens[b] >= 1 && prompt_lens[b] <= max_prompt, "decode_greedy: prompt_lens[%d]=%d out of range", b, prompt_lens[b]);
    CCX_REQUIRE(ctx, prompt_lens[b] + sample_len - 1 <= w->d.n_text_ctx, "decode_greedy: prompt %d + sample_len %d exceeds n_text_ctx", prompt_lens[b], sample_len);
    CCX_REQUIRE(ctx, prompt_lens[b] > w->sot_tail + w->prefix_len, "decode: prompt_lens[%d] = %d does not hold a SOT sequence of 1 + %d tokens (ccx_whisper_set_sot_tail) and a prefix of %d (ccx_whisper_set_prefix_len)", b,
                prompt_lens[b], w->sot_tail, w->prefix_len);
    for (int i = 0; i < prompt_lens[b]; i++) {
      const int t = prompt_ids[(size_t)b * max_prompt + i];
      CCX_REQUIRE(ctx, t >= 0 && t < w->d.n_vocab, "decode_greedy: prompt token %d out of range", t);
    }
    if (prompt_lens[b] > *max_pl) *max_pl = prompt_lens[b];
  }
  return CCX_OK;
}

// (2) the row -> window map and the stream ids of a mapped decode: uploaded once per call (the state upload synchronises)
int upload_row_map(ccx_whisper* w, const int32_t* win, const int32_t* sids, int B, hipStream_t stream) {
  if (!w->row_win) {
    CCX_TRY(w->store.alloc(&w->row_win, (size_t)w->max_batch, true));
    CCX_TRY(w->store.alloc(&w->row_sid, (size_t)w->max_batch, true));
    CCX_TRY(w->store.alloc(&w->pf_win, (size_t)w->max_batch * ccx_whisper::kPrefillMax, true));
  }
  CCX_HIP(w->ctx, hipMemcpyAsync(w->row_win, win, (size_t)B * 4, hipMemcpyHostToDevice, stream));
  if (sids) CCX_HIP(w->ctx, hipMemcpyAsync(w->row_sid, sids, (size_t)B * 4, hipMemcpyHostToDevice, stream));
  return CCX_OK;
}

// (2) a beam decode's workspaces (first use), its cache indirection and finished counts, and a traced call's buffers
int setup_beam(ccx_whisper* w, const BeamCall& beam, int B, int sample_len, hipStream_t stream, BeamWork* bw) {
  ccx_ctx* ctx = w->ctx;
  const int Tc = w->d.n_text_ctx;
  if (!w->beam_ind) {
    const size_t mb = (size_t)w->max_batch;
    CCX_TRY(w->store.alloc(&w->beam_ind, mb * Tc, true));
    CCX_TRY(w->store.alloc(&w->beam_cand_id, mb * (kBeamMax + 1), true));
    CCX_TRY(w->store.alloc(&w->beam_cand_lp, mb * (kBeamMax + 1), true));
    CCX_TRY(w->store.alloc(&w->beam_fin_tok, mb * kBeamCandMax * w->sample_cap, true));
    CCX_TRY(w->store.alloc(&w->beam_fin_score, mb * kBeamCandMax, true));
    CCX_TRY(w->store.alloc(&w->beam_fin_n, mb * kBeamCandMax, true));
    CCX_TRY(w->store.alloc(&w->beam_fin_count, mb, true));
  }
  // after the prefill every row's keys are its own: ind[r][t] = r (the update kernel rewrites a row's entries from its parent's)
  bw->ind_init.resize((size_t)B * Tc);
  for (int r = 0; r < B; r++)
    for (int t = 0; t < Tc; t++) bw->ind_init[(size_t)r * Tc + t] = (unsigned short)r;
  CCX_HIP(ctx, hipMemcpyAsync(w->beam_ind, bw->ind_init.data(), bw->ind_init.size() * 2, hipMemcpyHostToDevice, stream));
  CCX_HIP(ctx, hipMemsetAsync(w->beam_fin_count, 0, (size_t)beam.G * 4, stream));
  if (beam.trace) {
    const size_t n = (size_t)sample_len * B, K = (size_t)beam.beam + 1;
    BeamTrace& t = bw->trace;
    const size_t bytes[5] = {n * K * 4, n * K * 4, n * 4, n * 4, n * 4};
    void** bufs[5] = {(void**)&t.cid, (void**)&t.clp, (void**)&t.tok, (void**)&t.par, (void**)&t.score};
    for (int i = 0; i < 5; i++) CCX_HIP(ctx, hipMalloc(bufs[i], bytes[i]));
    for (int i = 0; i < 5; i++) CCX_HIP(ctx, hipMemsetAsync(*bufs[i], 0xFF, bytes[i], stream));
  }
  return CCX_OK;
}

// (4) The lane policy: the row ranges [b0, b0 + B) that step concurrently.  `forced`: CCX_DEC_LANES (0: the default below);
// `max_lanes`: kMaxLanes, or the concurrent streams the probe found.
struct RowRange { int b0, B; };
std::vector<RowRange> lane_policy(int B, bool xs_on, bool beam, int forced, int max_lanes) {
  int nl = 1;
  if (forced >= 1) nl = forced;
  // measured at 192 sequences x 65 steps: 1 lane 292.5, 2 286.8, 3 284.9, 4 284.8 ms; pipeline step with 384-sequence groups: 2 lanes
  // 710.0, 3 lanes 698.0 ms; with 768-sequence groups: 1 lane 721.5, 2 lanes 676.6, 3 lanes 687.5, 4 lanes 704.0 ms
  // with the cross attention against the encoder output (half the bytes: the chain weighs more): 768-sequence groups 2 lanes 561.3,
  // 3 lanes 557.9 ms per pipeline step
  // ... 384-sequence groups 3 lanes 598.6, 2 lanes 616.6 ms; 192-sequence groups (the sequential schedule) 1 lane 768.1, 2 lanes
  // 779.5, 3 lanes 793.2 ms: below ~128 rows per lane the streaming launches no longer fill the chip
  else if (xs_on) nl = B >= 320 ? 3 : 1;
  else nl = B >= 640 ? 2 : (B >= 144 ? 3 : (B >= 96 ? 2 : 1));
  if (nl > max_lanes) nl = max_lanes;
  while (nl > 1 && B / nl < 16) nl--;
  if (beam) nl = 1;      // a window's rows are rewritten by one block and counted by one n_done: one lane
  const int per = ccx_cdiv(ccx_cdiv(B, nl), 16) * 16;   // lane sizes in multiples of one MFMA row tile
  std::vector<RowRange> r;
  for (int b0 = 0; (int)r.size() < nl && b0 < B; b0 += per) r.push_back({b0, b0 + per <= B ? per : B - b0});
  return r;
}

// (4) the lanes of a decode: the policy's ranges (fewer if the probe finds fewer concurrent streams), each with the decode's plan
// narrowed to its rows and with its own stream, logits rows and done counter.  Sets base.cross_lds_pad, which the lanes share.
int plan_lanes(ccx_whisper* w, StepPlan& base, hipStream_t stream, const BeamTrace* trace, Lanes* L) {
  const char* e = getenv("CCX_DEC_LANES");
  const int forced = e ? atoi(e) : 0;
  const bool beam = base.beam_size > 0;
  std::vector<RowRange> rows = lane_policy(base.B, w->xs_on, beam, forced, ccx_whisper::kMaxLanes);
  const std::vector<hipStream_t>* extra = nullptr;
  if (rows.size() > 1) {
    extra = &lane_streams_for(w, stream);
    if (extra->size() + 1 < rows.size()) rows = lane_policy(base.B, w->xs_on, beam, forced, (int)extra->size() + 1);
  }
  // While lanes overlap, the cross attention of one lane (4,608 short blocks that fill every wave slot) makes the other
  // lanes' 5-8 us kernels queue for a slot.  Its blocks therefore claim 64 KB of LDS they do not use: two blocks per CU
  // still keep HBM saturated (each wave has 16 KB of loads in flight; 49.4 -> 51.3 us per launch) and the pipeline step
  // drops 924 -> 897 ms (3 blocks per CU: 910; 4: 919; 1: 979).
  // Lean streaming: ONE 4-wave block per CU (98 KB of claimed LDS), each wave with 8-16 KB in flight.  The claim only exists to
  // leave room for the OTHER lanes' chain kernels: a single lane runs uncapped.
  base.cross_lds_pad = rows.size() > 1 ? 98304 : 0;
  const long ld = w->Vpad;
  L->n = (int)rows.size();
  for (int i = 0; i < L->n; i++) {
    Lane& l = L->lane[i];
    l.plan = base;
    l.plan.b0 = rows[i].b0; l.plan.B = rows[i].B; l.plan.lane_idx = i; l.plan.select = 1;
    l.io = StepIo{};
    l.io.logits = w->dlogits + (long)rows[i].b0 * ld; l.io.ld = ld; l.io.n_done = w->n_done + i;
    l.io.stream = i == 0 ? stream : (*extra)[i - 1];
    l.io.trace = trace;
    l.exec = nullptr;
  }
  return CCX_OK;
}

// (5) the prompt prefill, the no-speech probability at the SOT position and the first sample of every sequence, all on `stream`
int prefill_and_first_sample(ccx_whisper* w, const StepPlan& base, const Lanes& L, const int32_t* win, const int32_t* prompt_ids,
                             const int32_t* prompt_lens, int max_pl, hipStream_t stream) {
  CCX_TRY(run_prefill(w, base, win, prompt_ids, prompt_lens, max_pl, stream));
  // no-speech probability from the raw logits at the SOT position, over the ids of the vocabulary (eager, before the captured steps;
  // w->dlogits is free until the first sample below)
  if (w->ns_at_sot()) CCX_TRY(token_probs_of_rows(w, w->tp_xn, base.B, 0, w->d.n_vocab, w->rules.no_speech, nullptr, stream));
  // first sample of every sequence, lane by lane (each lane counts its own finished sequences)
  for (int i = 0; i < L.n; i++) {
    StepIo io = L.lane[i].io;
    io.stream = stream;
    CCX_TRY(dec_head(w, L.lane[i].plan, io));
  }
  return CCX_OK;
}

// (6) The first step runs eagerly (also performs one-time kernel attribute setup outside of capture).  Lane i + 1
// starts when lane i reaches its first cross attention, which sets the stagger the later steps keep.
int first_step_eager(ccx_whisper* w, const Lanes& L, bool sync_lanes) {
  for (int i = 0; i < L.n; i++) {
    StepIo io = L.lane[i].io;
    if (i > 0) CCX_HIP(w->ctx, hipStreamWaitEvent(io.stream, w->lane_start[i - 1], 0));
    io.stagger = (i + 1 < L.n) ? w->lane_start[i] : nullptr;
    CCX_TRY(dec_step(w, L.lane[i].plan, io));
    if (sync_lanes) CCX_HIP(w->ctx, hipStreamSynchronize(io.stream));
  }
  return CCX_OK;
}

// (7) The step graph of a lane: the cached one of its plan, or captured now -- the only place that captures.  The plan is
// everything a captured step depends on besides instance constants (StepPlan); the per-call buffers io can carry are not in it,
// so a step with such buffers is never captured.
int step_graph(ccx_whisper* w, Lane& lane) {
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, !lane.io.align && !lane.io.trace && !lane.io.stagger, "step_graph: a step with per-call buffers cannot be captured");
  auto it = w->graphs.find(lane.plan);
  if (it != w->graphs.end()) { lane.exec = it->second; return CCX_OK; }
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  CCX_HIP(ctx, hipStreamBeginCapture(lane.io.stream, hipStreamCaptureModeThreadLocal));
  int rc = dec_step(w, lane.plan, lane.io);
  hipError_t e = hipStreamEndCapture(lane.io.stream, &graph);
  if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
  if (e != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (e != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  w->graphs[lane.plan] = exec;
  lane.exec = exec;
  return CCX_OK;
}

// (8) The steps [step, total_steps), queued in chunks; the done counters of chunk c are polled only after chunk c + 1 is queued,
// so no stream runs dry while the host waits.  Ends early once every sequence of every lane is done.
int run_chunks(ccx_whisper* w, const Lanes& L, int step, int total_steps, bool sync_lanes) {
  ccx_ctx* ctx = w->ctx;
  const int kChunk = 8, nl = L.n;
  auto queue_chunk = [&](int c, int n) -> int {
    for (int k = 0; k < n; k++)
      for (int i = 0; i < nl; i++) {
        const Lane& l = L.lane[i];
        if (l.exec) CCX_HIP(ctx, hipGraphLaunch(l.exec, l.io.stream));   // ~50 us of host time per replay
        else {
          CCX_TRY(dec_step(w, l.plan, l.io));
          // eager profiling runs (ccx_prof_enable + CCX_NO_GRAPH) time every kernel with an event pair: keep the lanes apart so
          // that the durations are those of the kernel alone, as rocprofv3 (which serialises replays) sees them
          if (sync_lanes) CCX_HIP(ctx, hipStreamSynchronize(l.io.stream));
        }
      }
    for (int i = 0; i < nl; i++) {
      CCX_HIP(ctx, hipMemcpyAsync(&w->poll_host[(c & 1) * ccx_whisper::kMaxLanes + i], w->n_done + i, 4, hipMemcpyDeviceToHost, L.lane[i].io.stream));
      CCX_HIP(ctx, hipEventRecord(w->lane_poll[c & 1][i], L.lane[i].io.stream));
    }
    return CCX_OK;
  };
  auto chunk_done = [&](int c, bool* all) -> int {
    *all = true;
    for (int i = 0; i < nl; i++) {
      CCX_HIP(ctx, hipEventSynchronize(w->lane_poll[c & 1][i]));
      if (w->poll_host[(c & 1) * ccx_whisper::kMaxLanes + i] < L.lane[i].plan.B) *all = false;
    }
    return CCX_OK;
  };
  int c = 0;
  bool pending = false;   // chunk c - 1 queued but not polled yet
  while (step < total_steps) {
    const int n = (total_steps - step < kChunk) ? total_steps - step : kChunk;
    CCX_TRY(queue_chunk(c, n));
    step += n;
    if (pending) {
      bool all;
      CCX_TRY(chunk_done(c - 1, &all));
      if (all) break;
    }
    pending = true;
    c++;
  }
  return CCX_OK;
}

// (10) append this decode's stamp trace: one line per lane "lane <i> <n> <stamp> ..." (stamp = realtime << 8 | tag), then reset
int dump_stamps(ccx_whisper* w, int B, int nl, hipStream_t stream) {
  ccx_ctx* ctx = w->ctx;
  CCX_HIP(ctx, hipStreamSynchronize(stream));
  std::vector<int> cnt(ccx_whisper::kMaxLanes);
  CCX_HIP(ctx, hipMemcpy(cnt.data(), w->stamp_count, cnt.size() * 4, hipMemcpyDeviceToHost));
  if (FILE* f = fopen(w->stamp_path.c_str(), "a")) {
    fprintf(f, "decode B %d lanes %d\n", B, nl);
    for (int i = 0; i < nl; i++) {
      const int n = cnt[i] < ccx_whisper::kStampCap ? cnt[i] : ccx_whisper::kStampCap;
      std::vector<unsigned long long> buf(n);
      CCX_HIP(ctx, hipMemcpy(buf.data(), w->stamps + (size_t)i * ccx_whisper::kStampCap, (size_t)n * 8, hipMemcpyDeviceToHost));
      fprintf(f, "lane %d %d", i, n);
      for (int k = 0; k < n; k++) fprintf(f, " %llu", buf[k]);
      fprintf(f, "\n");
    }
    fclose(f);
  }
  CCX_HIP(ctx, hipMemset(w->stamp_count, 0, ccx_whisper::kMaxLanes * 4));
  return CCX_OK;
}

// (11) what every decode reads back: the rows' final states, their sampled tokens, the no-speech probabilities taken at the SOT
struct RowsBack {
  std::vector<DecSeqState> st;
  std::vector<int> gen;
  std::vector<float> ns_sot;
};
int queue_rows_back(ccx_whisper* w, int B, int sample_len, hipStream_t stream, RowsBack* rb) {
  rb->st.resize(B);
  rb->gen.resize((size_t)B * sample_len);
  rb->ns_sot.resize(w->ns_at_sot() ? B : 0);
  CCX_HIP(w->ctx, hipMemcpyAsync(rb->st.data(), w->state, B * sizeof(DecSeqState), hipMemcpyDeviceToHost, stream));
  if (w->ns_at_sot()) CCX_HIP(w->ctx, hipMemcpyAsync(rb->ns_sot.data(), w->tp_prob, (size_t)B * 4, hipMemcpyDeviceToHost, stream));
  CCX_HIP(w->ctx, hipMemcpyAsync(rb->gen.data(), w->gen, rb->gen.size() * 4, hipMemcpyDeviceToHost, stream));
  return CCX_OK;
}

// (11) a plain or mapped decode: one result per row
int read_back_rows(ccx_whisper* w, int B, int sample_len, hipStream_t stream, int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out,
                   float* no_speech_prob_out) {
  RowsBack rb;
  CCX_TRY(queue_rows_back(w, B, sample_len, stream, &rb));
  CCX_HIP(w->ctx, hipStreamSynchronize(stream));
  const std::vector<DecSeqState>& st = rb.st;
  for (int b = 0; b < B; b++) {
    const int ng = st[b].n_gen < sample_len ? st[b].n_gen : sample_len;
    // not done after the step budget: treat everything sampled as text (no eot was produced)
    const int ntok = st[b].done ? st[b].n_tokens : ng;
    for (int i = 0; i < sample_len; i++) tokens_out[(size_t)b * sample_len + i] = (i < ntok) ? rb.gen[(size_t)b * sample_len + i] : w->rules.eot;
    if (n_tokens_out) n_tokens_out[b] = ntok;
    if (sum_logprob_out) sum_logprob_out[b] = st[b].sum_logprob;
    // (the select kernel's value is that of the LAST prompt position over the ids rounded up to 4: replaced where that is not the rule)
    if (no_speech_prob_out) no_speech_prob_out[b] = w->ns_at_sot() ? rb.ns_sot[b] : st[b].no_speech_prob;
  }
  return CCX_OK;
}

// (11) a beam decode -- BeamSearchDecoder.finalize: per window the finished hypotheses in insertion order, topped up with the live
// rows by descending score; tokens_out / n_tokens_out / sum_logprob_out are [G][C][sample_len] / [G][C] / [G][C], C = max(beam, maxc)
int read_back_beam(ccx_whisper* w, const BeamCall& beam, const BeamTrace& trace, int B, int sample_len, hipStream_t stream, int32_t* tokens_out,
                   int32_t* n_tokens_out, float* sum_logprob_out, float* no_speech_prob_out) {
  ccx_ctx* ctx = w->ctx;
  RowsBack rb;
  CCX_TRY(queue_rows_back(w, B, sample_len, stream, &rb));
  const std::vector<DecSeqState>& st = rb.st;
  const int G = beam.G, bs = beam.beam, mc = beam.maxc, C = bs > mc ? bs : mc, eot = w->rules.eot;
  std::vector<int> fin_tok((size_t)G * mc * sample_len), fin_n((size_t)G * mc), fin_count(G);
  std::vector<float> fin_score((size_t)G * mc);
  CCX_HIP(ctx, hipMemcpyAsync(fin_tok.data(), w->beam_fin_tok, fin_tok.size() * 4, hipMemcpyDeviceToHost, stream));
  CCX_HIP(ctx, hipMemcpyAsync(fin_n.data(), w->beam_fin_n, fin_n.size() * 4, hipMemcpyDeviceToHost, stream));
  CCX_HIP(ctx, hipMemcpyAsync(fin_score.data(), w->beam_fin_score, fin_score.size() * 4, hipMemcpyDeviceToHost, stream));
  CCX_HIP(ctx, hipMemcpyAsync(fin_count.data(), w->beam_fin_count, (size_t)G * 4, hipMemcpyDeviceToHost, stream));
  CCX_HIP(ctx, hipStreamSynchronize(stream));
  if (const ccx_beam_trace* tr = beam.trace) {
    const size_t n = (size_t)sample_len * B, K = (size_t)bs + 1;
    CCX_HIP(ctx, hipMemcpy(tr->cand_id, trace.cid, n * K * 4, hipMemcpyDeviceToHost));
    CCX_HIP(ctx, hipMemcpy(tr->cand_lp, trace.clp, n * K * 4, hipMemcpyDeviceToHost));
    CCX_HIP(ctx, hipMemcpy(tr->tok, trace.tok, n * 4, hipMemcpyDeviceToHost));
    CCX_HIP(ctx, hipMemcpy(tr->parent, trace.par, n * 4, hipMemcpyDeviceToHost));
    CCX_HIP(ctx, hipMemcpy(tr->score, trace.score, n * 4, hipMemcpyDeviceToHost));
  }
  for (int g = 0; g < G; g++) {
    int n_hyp = 0;
    auto put = [&](const int* toks, int n, float score) {
      const size_t at = (size_t)g * C + n_hyp;
      for (int i = 0; i < sample_len; i++) tokens_out[at * sample_len + i] = i < n ? toks[i] : eot;
      if (n_tokens_out) n_tokens_out[at] = n;
      if (sum_logprob_out) sum_logprob_out[at] = score;
      n_hyp++;
    };
    const int nf = fin_count[g] < mc ? fin_count[g] : mc;
    for (int k = 0; k < nf; k++) {
      const size_t slot = (size_t)g * mc + k;
      put(&fin_tok[slot * sample_len], fin_n[slot], fin_score[slot]);
    }
    if (n_hyp < bs) {
      std::vector<int> rows(bs);
      for (int j = 0; j < bs; j++) rows[j] = g * bs + j;
      std::stable_sort(rows.begin(), rows.end(), [&](int a, int b) { return st[a].sum_logprob > st[b].sum_logprob; });
      for (int j = 0; j < bs && n_hyp < bs; j++) {
        const int r = rows[j];
        const int ng = st[r].n_gen < sample_len ? st[r].n_gen : sample_len;
        put(&rb.gen[(size_t)r * sample_len], ng, st[r].sum_logprob);
      }
    }
    for (int k = n_hyp; k < C; k++) {          // unused slots: empty
      const size_t at = (size_t)g * C + k;
      for (int i = 0; i < sample_len; i++) tokens_out[at * sample_len + i] = eot;
      if (n_tokens_out) n_tokens_out[at] = 0;
      if (sum_logprob_out) sum_logprob_out[at] = 0.f;
    }
    if (beam.n_hyp_out) beam.n_hyp_out[g] = n_hyp;
    if (no_speech_prob_out) no_speech_prob_out[g] = w->ns_at_sot() ? rb.ns_sot[(size_t)g * bs] : st[(size_t)g * bs].no_speech_prob;
  }
  return CCX_OK;
}

// The decode behind ccx_whisper_decode (win == NULL: row r reads window r, noise stream r) and ccx_whisper_decode_rows (B rows over
// n_windows encoded windows: row r reads window win[r]; sids, if given, names every row's noise stream).  Both checked by the callers.
// beam != NULL (ccx_whisper_decode_beam): the B rows are beam->G windows of beam->beam rows over the map (read_back_beam).
int decode_impl(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int B, int sample_len,
                float temperature, uint64_t seed, int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out,
                float* no_speech_prob_out, void* stream_, const int32_t* win, int n_windows, const int32_t* sids,
                const BeamCall* beam = nullptr) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  hipStream_t stream = (hipStream_t)stream_;
  int max_pl = 0;
  CCX_TRY(check_decode_args(w, prompt_ids, prompt_lens, max_prompt, B, sample_len, temperature, tokens_out, &max_pl));
  CCX_TRY(own_stream_if_null(w, &stream));
  // prompts of 2 tokens and more are prefilled, kPrefillMax positions per pass (CCX_PREFILL=0: one decode step per prompt token, round
  // 1's way)
  const int prefill_on = [] { const char* e = getenv("CCX_PREFILL"); return e ? atoi(e) : 1; }();     // read per call: tests flip it
  // ... and every prompt of an instance that reads its no-speech probability at the SOT position with the ranged softmax
  const bool ns_at_sot = w->ns_at_sot();
  CCX_REQUIRE(ctx, !ns_at_sot || prefill_on, "decode: CCX_PREFILL=0 is not available on an instance with a SOT tail (%d) or with n_vocab = %d, no multiple of 4: "
              "its no-speech probability is taken from the prefill", w->sot_tail, w->d.n_vocab);
  const bool prefill = prefill_on && (max_pl >= 2 || ns_at_sot);
  if (ns_at_sot) CCX_TRY(ensure_token_probs_scratch(w));

  // the plan of the whole decode: the lanes narrow it to their rows, the prefill takes it as it is
  StepPlan base{};
  base.B = B; base.sample_len = sample_len; base.max_prompt = max_prompt; base.sampling = temperature > 0.f;
  base.cross_stream = 1;
  base.map_on = win != nullptr; base.sid_on = win && sids;
  if (beam) { base.beam_size = beam->beam; base.beam_maxc = beam->maxc; }
  base.stamp_level = w->stamps_on ? w->stamp_level : 0;
  // the call's options: a default decode keeps the plan it always had (the rules' mask and index, the ruled kernels)
  base.max_init_ts = w->rules.max_initial_timestamp_index;
  if (w->opts_on) {
    base.opt_mask = 1; base.no_ts = w->opts.without_timestamps != 0; base.sup_blank = w->opts.suppress_blank != 0;
    if (w->opts.max_initial_timestamp_index != -2) base.max_init_ts = w->opts.max_initial_timestamp_index;
    if (base.no_ts) base.max_init_ts = -1;         // not read without the rules: one plan whatever the caller left there
  }
  // the history rules: {1.0, 0}, set or not, is the default plan
  base.hist_ngram = w->hist.no_repeat_ngram_size;
  if (w->hist.repetition_penalty != 1.0f) memcpy(&base.hist_pen_bits, &w->hist.repetition_penalty, 4);
  base.bias_on = w->bias_on ? 1 : 0;      // no table, set or not, is the default plan
  // truncated sampling: {0, 1.0, 0.0}, set or not, and every decode at temperature 0 (greedy, beam) is the plan it always was
  base.trunc_on = (base.sampling && (w->trunc.top_k != 0 || w->trunc.top_p != 1.0f || w->trunc.min_p != 0.0f)) ? 1 : 0;
  // per-token log-probabilities: off, set or not, and every beam decode is the plan it always was
  base.logp = (!beam && w->logp_n >= 0) ? 1 + w->logp_n : 0;
  w->logp_top = -1;
  if (base.logp) {
    // what no sampled step writes reads NaN, -1 and -inf (on `stream`, ahead of the state upload every lane waits for)
    const size_t n = (size_t)B * sample_len;
    CCX_HIP(ctx, hipMemsetAsync(w->tok_lp, 0xFF, n * 4, stream));
    CCX_HIP(ctx, hipMemsetAsync(w->top_id, 0xFF, n * CCX_LOGPROB_MAX_TOP * 4, stream));
    CCX_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)w->top_lp, (int)0xFF800000u, n * CCX_LOGPROB_MAX_TOP, stream));
    w->logp_R = B; w->logp_SL = sample_len; w->logp_top = w->logp_n;
  }
  read_chain_switches(w, base);
  CCX_TRY(select_cross_path(w, base, stream, win ? n_windows : -1));
  if (win) CCX_TRY(upload_row_map(w, win, sids, B, stream));
  BeamWork bw;
  if (beam) {
    CCX_REQUIRE(ctx, prefill_on, "ccx_whisper_decode_beam: CCX_PREFILL=0 is not available to a beam decode (its kernels have no prompt phase)");
    CCX_TRY(setup_beam(w, *beam, B, sample_len, stream, &bw));
  }
  CCX_TRY(upload_decode_state(w, prompt_ids, prompt_lens, max_prompt, B, temperature, seed, stream, prefill));

  Lanes L;
  CCX_TRY(plan_lanes(w, base, stream, bw.trace.cid ? &bw.trace : nullptr, &L));
  // which cross attention the steps of this decode run (lane 0; a short last lane of <= 16 rows takes the <= 16-row kernels of its path)
  w->last_cross_path = base.xs_active ? 2 : (L.lane[0].plan.B > 16 ? 1 : 0);
  // steps still to run after the (eager) first one: the prefill already covers the prompt AND takes the first sample
  const int total_steps = prefill ? sample_len : max_pl - 1 + sample_len;
  const bool use_graph = getenv("CCX_NO_GRAPH") == nullptr && !L.lane[0].io.trace;   // (a traced beam decode: per-call buffers)
  const bool sync_lanes = ctx->prof_on && !use_graph && L.n > 1;     // eager profiling runs: see run_chunks

  if (prefill) CCX_TRY(prefill_and_first_sample(w, base, L, win, prompt_ids, prompt_lens, max_pl, stream));
  // the state upload (and the prefill) was queued on `stream`: the other lanes start after it
  CCX_HIP(ctx, hipEventRecord(w->own_event, stream));
  for (int i = 1; i < L.n; i++) CCX_HIP(ctx, hipStreamWaitEvent(L.lane[i].io.stream, w->own_event, 0));
  int step = prefill ? 1 : 0;                   // the prefill's own sample counts as step 0
  if (step < total_steps) {
    CCX_TRY(first_step_eager(w, L, sync_lanes));
    step += 1;
  }
  if (use_graph && step < total_steps)
    for (int i = 0; i < L.n; i++) CCX_TRY(step_graph(w, L.lane[i]));
  CCX_TRY(run_chunks(w, L, step, total_steps, sync_lanes));
  // join the lanes back into `stream`
  for (int i = 1; i < L.n; i++) {
    CCX_HIP(ctx, hipEventRecord(w->lane_start[i], L.lane[i].io.stream));
    CCX_HIP(ctx, hipStreamWaitEvent(stream, w->lane_start[i], 0));
  }
  if (w->stamps_on) CCX_TRY(dump_stamps(w, B, L.n, stream));
  if (beam) return read_back_beam(w, *beam, bw.trace, B, sample_len, stream, tokens_out, n_tokens_out, sum_logprob_out, no_speech_prob_out);
  return read_back_rows(w, B, sample_len, stream, tokens_out, n_tokens_out, sum_logprob_out, no_speech_prob_out);
}

}  // namespace

extern "C" {

int ccx_whisper_decode(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int B, int sample_len,
                       float temperature, uint64_t seed, int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out,
                       float* no_speech_prob_out, void* stream_) {
  return decode_impl(w, prompt_ids, prompt_lens, max_prompt, B, sample_len, temperature, seed, tokens_out, n_tokens_out, sum_logprob_out,
                     no_speech_prob_out, stream_, nullptr, 0, nullptr);
}

int ccx_whisper_decode_rows(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int R,
                            const int32_t* window_of_row, int n_windows, const int32_t* stream_ids, int sample_len, float temperature,
                            uint64_t seed, int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out, float* no_speech_prob_out,
                            void* stream_) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->finalized && w->rules_set, "ccx_whisper_decode_rows: not finalized or rules not set");
  CCX_REQUIRE(ctx, R >= 1 && R <= w->max_batch, "ccx_whisper_decode_rows: R = %d out of range [1, max_batch = %d]", R, w->max_batch);
  CCX_REQUIRE(ctx, window_of_row != nullptr, "ccx_whisper_decode_rows: window_of_row is NULL");
  CCX_REQUIRE(ctx, n_windows >= 1 && n_windows <= w->max_batch, "ccx_whisper_decode_rows: n_windows = %d out of range [1, max_batch = %d]", n_windows,
              w->max_batch);
  CCX_REQUIRE(ctx, n_windows <= w->enc_B, "ccx_whisper_decode_rows: n_windows = %d, the last ccx_whisper_encode left %d windows", n_windows, w->enc_B);
  for (int r = 0; r < R; r++) {
    CCX_REQUIRE(ctx, window_of_row[r] >= 0 && window_of_row[r] < n_windows, "ccx_whisper_decode_rows: window_of_row[%d] = %d out of range [0, n_windows = %d)", r,
                window_of_row[r], n_windows);
    if (stream_ids) CCX_REQUIRE(ctx, stream_ids[r] >= 0, "ccx_whisper_decode_rows: stream_ids[%d] = %d is negative", r, stream_ids[r]);
  }
  return decode_impl(w, prompt_ids, prompt_lens, max_prompt, R, sample_len, temperature, seed, tokens_out, n_tokens_out, sum_logprob_out,
                     no_speech_prob_out, stream_, window_of_row, n_windows, stream_ids);
}

int ccx_whisper_decode_beam(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int G,
                            const int32_t* window_of_group, int n_windows, int beam_size, int max_candidates, int sample_len,
                            int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out, int32_t* n_hyp_out,
                            float* no_speech_prob_out, const ccx_beam_trace* trace, void* stream_) {
  if (!w) return CCX_ERR_ARG;
  ccx_ctx* ctx = w->ctx;
  CCX_REQUIRE(ctx, w->finalized && w->rules_set, "ccx_whisper_decode_beam: not finalized or rules not set");
  CCX_REQUIRE(ctx, beam_size >= 1 && beam_size <= kBeamMax, "ccx_whisper_decode_beam: beam_size = %d out of range [1, %d]", beam_size, kBeamMax);
  CCX_REQUIRE(ctx, max_candidates >= 1 && max_candidates <= kBeamCandMax, "ccx_whisper_decode_beam: max_candidates = %d out of range [1, %d]", max_candidates,
              kBeamCandMax);
  CCX_REQUIRE(ctx, G >= 1 && (long)G * beam_size <= w->max_batch, "ccx_whisper_decode_beam: G = %d, G * beam_size must lie in [1, max_batch = %d]", G, w->max_batch);
  CCX_REQUIRE(ctx, n_windows >= 1 && n_windows <= w->max_batch, "ccx_whisper_decode_beam: n_windows = %d out of range [1, max_batch = %d]", n_windows, w->max_batch);
  CCX_REQUIRE(ctx, n_windows <= w->enc_B, "ccx_whisper_decode_beam: n_windows = %d, the last ccx_whisper_encode left %d windows", n_windows, w->enc_B);
  CCX_REQUIRE(ctx, prompt_ids && prompt_lens && tokens_out && max_prompt >= 1 && max_prompt <= w->max_prompt_cap, "ccx_whisper_decode_beam: prompt_ids, prompt_lens or tokens_out is NULL, or max_prompt = %d out of range",
              max_prompt);
  CCX_REQUIRE(ctx, window_of_group || G <= n_windows, "ccx_whisper_decode_beam: window_of_group is NULL with more groups (%d) than windows (%d)", G, n_windows);
  if (trace)
    CCX_REQUIRE(ctx, trace->n_steps >= sample_len && trace->cand_id && trace->cand_lp && trace->tok && trace->parent && trace->score,
                "ccx_whisper_decode_beam: trace.n_steps = %d below sample_len = %d, or a trace buffer is NULL", trace->n_steps, sample_len);
  const int R = G * beam_size;
  std::vector<int32_t> ids((size_t)R * max_prompt), lens(R), win(R);
  for (int g = 0; g < G; g++) {
    const int wg = window_of_group ? window_of_group[g] : g;
    CCX_REQUIRE(ctx, wg >= 0 && wg < n_windows, "ccx_whisper_decode_beam: window_of_group[%d] = %d out of range [0, n_windows = %d)", g, wg, n_windows);
    for (int j = 0; j < beam_size; j++) {
      const int r = g * beam_size + j;
      memcpy(&ids[(size_t)r * max_prompt], &prompt_ids[(size_t)g * max_prompt], (size_t)max_prompt * 4);
      lens[r] = prompt_lens[g]; win[r] = wg;
    }
  }
  const BeamCall bc{G, beam_size, max_candidates, n_hyp_out, trace};
  return decode_impl(w, ids.data(), lens.data(), max_prompt, R, sample_len, 0.f, 0, tokens_out, n_tokens_out, sum_logprob_out, no_speech_prob_out,
                     stream_, win.data(), n_windows, nullptr, &bc);
}

}  // extern "C"

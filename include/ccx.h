/* ccx.h -- C ABI of libccx, the MI355X-native (gfx950) compute library behind
 * ClearConverse's overlapped-speech transcription path.
 *
 * The reference has NO FFI for this path: EnhancedAudioProcessor calls duck-typed Python model
 * objects (reference back/api.py:657-797 creates them, back/api.py:1298-1549 drives them).  Each
 * entry point below states which of those Python calls it replaces; clearconverse_amd/_lib.py is
 * the ctypes binding and INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: every function returns 0 (CCX_OK) or a non-zero status and stores a message
 * retrievable with ccx_last_error(ctx).  All `*_dev` pointers are HIP device pointers owned by the
 * caller (torch allocates them); `stream` is a hipStream_t passed as void*.  The library owns only
 * weights, caches, workspaces and graphs inside its handles; it has no global state and starts no
 * threads, so it is safe to initialise after fork (reference back/api.py:2045-2049 forks per task).
 */
#ifndef CCX_H
#define CCX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CCX_DTYPE_F32 0
#define CCX_DTYPE_BF16 1
#define CCX_DTYPE_F16 2

typedef struct ccx_ctx ccx_ctx;
typedef struct ccx_whisper ccx_whisper;

const char* ccx_version(void);
int ccx_ctx_create(int device, ccx_ctx** out);
void ccx_ctx_destroy(ccx_ctx* ctx);
/* Last error text of this context ("" if none). ctx == NULL returns the text of the last failed
 * ccx_ctx_create on this thread. */
const char* ccx_last_error(const ccx_ctx* ctx);

/* ---- per-launch timing (HIP events on the launch stream) used by bench.py's roofline ----------
 * While enabled, every eagerly launched kernel of the library records a start/stop event pair and
 * its algorithmic flops/bytes.  Launches inside a stream capture (graph replay) are not recorded. */
int ccx_prof_enable(ccx_ctx* ctx, int on);  /* also clears previous records */
int ccx_prof_count(ccx_ctx* ctx);
int ccx_prof_get(ccx_ctx* ctx, int i, char* name_out, int name_cap, double* flops, double* bytes, float* ms);

/* ---- primitive operators (exposed so tests/ can check each kernel against oracle/) ------------ */

/* C[M,N] = A[M,K] * W[N,K]^T (+bias) with a fused epilogue; bf16 inputs, fp32 accumulate (MFMA).
 * epi: 0 bf16 out | 1 bf16 gelu | 2 f32 out = acc+bias+resid | 3 f32 out | 5 bf16 relu.
 * Replaces the torch.nn.Linear / Conv1d-as-GEMM calls inside whisper / speechbrain / pyannote
 * modules that the reference triggers at back/api.py:1077, 869, 1286. */
int ccx_gemm_bf16(ccx_ctx* ctx, int epi, const void* A_dev, int64_t lda, const void* W_dev, int64_t ldw,
                  const float* bias_dev, void* out_dev, int64_t ldo, const float* resid_dev, int64_t ldr,
                  int M, int N, int K, void* stream);

/* The full descriptor of the GEMM family (csrc/gemm_bf16.h GemmParams, field for field and in the same order; device pointers as
 * const void*), followed by the element count of every buffer.  See gemm_bf16.h for the meaning of each field. */
typedef struct ccx_gemm_desc {
  const void* A; const void* W;
  int64_t lda, ldw;
  int M, N, K;
  int ntaps; int64_t a_tap_stride;
  const void* bias;
  const void* out;
  int64_t ldo;
  const void* resid;
  int64_t ldr;
  int resid_mod;
  const void* scale; const void* shift;
  float slope;
  int rpb_in, rpb_out, roff, rpb_valid;
  int img_rows_in, img_rows_valid, img_rows_out;
  const void* resid_bf16; int64_t ldrb;
  const void* hq; const void* hk; const void* hv;
  int d_model, n_head;
  int S, Spad;
  int v_transposed;
  int first_block;
  /* elements (of the buffer's own type) that may be touched from each pointer above; heads_elems holds for each of hq / hk / hv */
  int64_t a_elems, w_elems, out_elems, resid_elems, resid_bf16_elems, heads_elems;
} ccx_gemm_desc;

/* Every epilogue (0 .. 8), tap, row-remap and operand-view path of the GEMM family from one descriptor -- the launches the model
 * handles make internally (conv stems, ResNet convolutions as shifted GEMMs, head-major Q/K/V, TDNN + BatchNorm).  Before the launch
 * the largest element index the kernel can touch in A, W, out, resid, resid_bf16 and hq / hk / hv is computed on the host and
 * compared with the stated counts: a descriptor that reaches past one of them is refused with CCX_ERR_ARG and a message naming the
 * buffer; nothing is launched.  For kernel parity tests. */
int ccx_gemm_bf16_desc(ccx_ctx* ctx, int epi, const ccx_gemm_desc* desc, void* stream);

/* LayerNorm over the last dim with fp32 statistics; writes bf16 and/or fp32 (either may be NULL). */
int ccx_layernorm(ccx_ctx* ctx, const float* x_dev, const float* gamma_dev, const float* beta_dev,
                  void* out_bf16_dev, float* out_f32_dev, int M, int D, float eps, void* stream);

/* Peak normalisation y = x / (max|x| + eps) per row (eps == 0: only when the peak is > 0) -- replaces
 * `signal_np / (np.max(np.abs(signal_np)) + 1e-8)` (reference back/api.py:834) and lines 350-351.
 * x,y [B, stride] f32 (may alias), n_samples_dev [B] int32 on the device. */
/* Ragged crops into a padded batch in one launch (the reference slices one crop at a time, `_extract_segment`,
 * back/api.py:840-860): dst[i][0 .. lens[i]) = row i, whose device address is src_ptrs_dev[i]; both tables in device memory. */
int ccx_gather_rows(ccx_ctx* ctx, const int64_t* src_ptrs_dev, const int* lens_dev, int n_rows, int max_len, float* dst_dev,
                    int64_t stride, void* stream);
int ccx_peak_normalize(ccx_ctx* ctx, const float* x_dev, float* y_dev, int64_t stride, const int* n_samples_dev, int B,
                       float eps, void* stream);
/* One decoder layer's cross attention as a stand-alone operator: out[r] = softmax(q[r] K^T / 8) V per head with K = xa Wk^T,
 * V = xa Wv^T + bv -- openai-whisper MultiHeadAttention.qkv_attention with xa (called per layer and decode step from
 * back/api.py:1286-1292 through transcribe()) -- computed the way the decode path of ccx_whisper_decode computes it for more than 80
 * sequences: against the encoder output itself (csrc/cross_x.hip), no K/V ever materialised.  q_dev [rows][64 n_head] f32 (bias
 * included), wk / wv [64 n_head][64 n_head] f32 and bv on the HOST, xa_dev bf16 [n_seq][n_ctx][64 n_head], row_seq (host, may be
 * null = identity) maps rows to sequences, out_dev [rows][64 n_head] f32.  rows_per_seq > 1: consecutive groups of that many rows
 * belong to one sequence each (the prompt prefill: four rows of a group then share one pass over the sequence's xa), else 0.
 * Synchronises the stream.  For kernel parity tests. */
int ccx_cross_attention_xa(ccx_ctx* ctx, const float* q_dev, const float* wk_host, const float* wv_host, const float* bv_host,
                           const uint16_t* xa_dev, const int* row_seq_host, int rows_per_seq, int rows, int n_seq, int n_head, int n_ctx,
                           float* out_dev, void* stream);
/* ---- FP8 encoder-output stream (opt-in, ccx_whisper_set_cross_fp8) --------------------------------------------------------------
 * The format (project-defined, MX-style).  Each key row of xa (D features, bf16) is quantised in blocks of 32 consecutive features:
 *   block scale   amax = the largest magnitude in the block.  The scale is 2^e, e the smallest integer with amax <= 448 * 2^e,
 *                 clamped to [-64, 64]; amax == 0 gives e = -64.  e is stored as one E8M0 byte, e + 127.  e comes from the exponent
 *                 bits of amax (frexp), not from a float log2.
 *   codes         code = e4m3fn(x / 2^e): OCP E4M3, round to nearest even, clamped to +-448 (only the clamp of e can make that bite).
 *   value         xhat = code * 2^e.  xhat is always exactly representable in bf16 (at most 4 significant bits, exponent within
 *                 bf16's range), so the FP8 stream computes, bit for bit, what the bf16 stream computes on xhat.
 *   inputs        finite (ln_post of finite activations).  NaN and Inf are NOT handled: their codes are unspecified.
 * Where the bytes sit in HBM (key order within a 16-key tile, the scale bytes, the padding of the last tile) is the streaming
 * kernel's business (csrc/xa_fp8.h); only the quantise kernel writes the image and only the stream and the read-back below read it.
 *
 * ccx_cross_attention_xa with the FP8 stream: xa_dev (not modified) is quantised with the model's quantise kernel, the three launches
 * run with the streaming kernel reading the image, and xhat_out_dev [n_seq][n_ctx][64 n_head] bf16 (required) receives xhat DECODED
 * FROM THE IMAGE by a read-back kernel, with the stream's own conversion.  out_dev is bit-identical to ccx_cross_attention_xa on
 * xhat_out_dev.  CCX_XS_FULL_LINES has no effect here.  Synchronises the stream.  For kernel parity tests. */
int ccx_cross_attention_xa_fp8(ccx_ctx* ctx, const float* q_dev, const float* wk_host, const float* wv_host, const float* bv_host,
                               const uint16_t* xa_dev, const int* row_seq_host, int rows_per_seq, int rows, int n_seq, int n_head,
                               int n_ctx, float* out_dev, uint16_t* xhat_out_dev, void* stream);
/* The two operators above with a key count PER SEQUENCE (reduced audio context, XsParams::seq_S of the streaming kernel): n_keys_host
 * [n_seq], each in [1, n_ctx]; sequence s is attended over its first n_keys_host[s] rows of xa only, and a row's output is, bit for
 * bit, what the plain operator gives for that sequence alone with n_ctx = n_keys_host[s].  The FP8 image is the one of all n_ctx
 * rows (no new format): the keys of a sequence's last 16-key tile beyond its count are real, finite rows whose weight is 0. */
int ccx_cross_attention_xa_keys(ccx_ctx* ctx, const float* q_dev, const float* wk_host, const float* wv_host, const float* bv_host,
                                const uint16_t* xa_dev, const int* row_seq_host, int rows_per_seq, int rows, int n_seq, int n_head,
                                int n_ctx, const int* n_keys_host, float* out_dev, void* stream);
int ccx_cross_attention_xa_fp8_keys(ccx_ctx* ctx, const float* q_dev, const float* wk_host, const float* wv_host, const float* bv_host,
                                    const uint16_t* xa_dev, const int* row_seq_host, int rows_per_seq, int rows, int n_seq, int n_head,
                                    int n_ctx, const int* n_keys_host, float* out_dev, uint16_t* xhat_out_dev, void* stream);
/* Embedding-quality weight of `_build_speaker_profiles`: out[b] = torch.var(x[b][0 .. n_b)) (unbiased; reference back/api.py:939).
 * fp64 accumulation in a fixed order: a row's value does not depend on its batch mates. */
int ccx_row_variance(ccx_ctx* ctx, const float* x_dev, int64_t stride, const int* n_samples_dev, int B, float* out_dev, void* stream);
/* `_calculate_embedding_similarity` (reference back/api.py:878-879: torch cosine_similarity(dim=0).item()), row-wise for a batch:
 * out[r] = sum_i (a[r][i] / max(|a[r]|, 1e-8)) * (b[r % b_rows][i] / max(|b[..]|, 1e-8)).  a [R, D], b [b_rows, D] f32. */
int ccx_cosine_rows(ccx_ctx* ctx, const float* a_dev, const float* b_dev, int R, int D, int b_rows, float* out_dev, void* stream);
/* The weighted sum of `_build_speaker_profiles` (reference back/api.py:946-953): out[c][s] = sum over turns t with spk[t] == s of
 * emb[c][t] * w[c][t] / (sum of those w[c][t]); NOT re-normalised.  emb [C, T, D], w [C, T], spk_dev [T] int32, out [C, S, D]. */
int ccx_speaker_profiles(ccx_ctx* ctx, const float* emb_dev, const float* w_dev, const int* spk_dev, int C, int T, int D, int S,
                         float* out_dev, void* stream);

/* K1: `torchaudio.transforms.Resample(orig_freq=sample_rate, new_freq=16000)(signal)` (reference back/api.py:824-830) with
 * torchaudio's default arguments.  orig / new_ are the two rates divided by their gcd, width = ceil(6 * orig / (min(orig, new_) * 0.99)),
 * kernT_dev the polyphase table TRANSPOSED, [2 * width + orig][new_] f32 (built by the caller exactly as upstream builds it:
 * clearconverse_amd/audio.py::sinc_resample_kernel).  x [B, stride_in] f32 rows of n_in_dev[b] samples -> y [B, stride_out] rows
 * of n_out_dev[b] = ceil(new_ * n_in / orig) samples; max_out = the largest of them.  All pointers are device pointers. */
int ccx_resample_sinc(ccx_ctx* ctx, const float* x_dev, int64_t stride_in, const int* n_in_dev, int B, int orig, int new_,
                      int width, const float* kernT_dev, float* y_dev, int64_t stride_out, const int* n_out_dev, int max_out,
                      void* stream);

/* Non-causal attention, head_dim 64 (Whisper encoder).  q,k: [B*H, Spad, 64] bf16 with rows >= S
 * zero; vt: [B*H, 64, Spad] bf16; o: [B*S, H*64] bf16.  Softmax scale 1/8 (= 64^-0.25 on q and k). */
int ccx_enc_attention(ccx_ctx* ctx, const void* q_dev, const void* k_dev, const void* vt_dev, void* o_dev,
                      int B, int H, int S, int Spad, void* stream);
/* The same with a key count per sequence (reduced audio context): n_keys_host [B], each in [1, S].  Sequence b attends over its first
 * n_keys_host[b] positions only; its rows of o below the count are, bit for bit, those of ccx_enc_attention on that sequence alone
 * with S = n_keys_host[b] (same Spad); its rows at or beyond the count are zeros.  Rows of q, k, vt between the count and Spad need
 * only be finite.  All counts equal to S: the bits of ccx_enc_attention.  Synchronises the stream.  For kernel parity tests. */
int ccx_enc_attention_keys(ccx_ctx* ctx, const void* q_dev, const void* k_dev, const void* vt_dev, void* o_dev,
                           int B, int H, int S, int Spad, const int* n_keys_host, void* stream);

/* ---- Whisper (replaces self.whisper_model, reference back/api.py:665-703; calls at
 *      back/api.py:1286-1292, 1432-1438, 1474-1480) ---------------------------------------------- */

typedef struct {
  int n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} ccx_whisper_dims;

/* Token-id constants of the tokenizer the checkpoint was trained with (openai-whisper
 * tokenizer.py; for *.en models sot=50257, eot=50256, ... see clearconverse_amd/tokenizer.py). */
typedef struct {
  int eot, sot, sot_prev, no_speech, no_timestamps, timestamp_begin, blank; /* blank = id of " " */
  int max_initial_timestamp_index;  /* 50 = 1.0 s; < 0 disables the rule */
  int n_suppress;
  const int* suppress;              /* host array, copied */
} ccx_decode_rules;

/* Accepted dims: n_audio_state == n_text_state, a multiple of 128 up to 1280 (tiny ... medium, and the 1280-wide large family), with
 * head_dim 64 on both sides; n_mels 80 or 128 (large-v3, large-v3-turbo); n_audio_ctx 1500; n_vocab in [4, 53248]; n_audio_layer and
 * n_text_layer >= 1, not necessarily equal (large-v3-turbo: 32 / 4).  max_batch in [1, 1536].  Widths above 768 (medium, the large
 * family) keep per-layer cross-attention K / V caches for all max_batch sequences: 2 x 1536 x n_state bf16 per decoder layer and
 * sequence (252 MB per sequence for a 1280-wide model with 32 decoder layers, 31 MB with 4). */
int ccx_whisper_create(ccx_ctx* ctx, const ccx_whisper_dims* dims, int max_batch, ccx_whisper** out);
void ccx_whisper_destroy(ccx_whisper* w);
/* Register one tensor by its openai-whisper state_dict name (the key layout of the reference's
 * fine-tune overlay, back/api.py:671-692), plus "mel_filters" [n_mels, 201].  data may be a host
 * or a device pointer.  Unknown names are an error. */
int ccx_whisper_set_tensor(ccx_whisper* w, const char* name, const void* data, int dtype, int ndim,
                           const int64_t* shape);
/* Longest clip (seconds) ccx_whisper_logmel must accept (default 30); call before finalize.  The log-mel of the
 * whole clip is normalised with its global maximum, exactly like whisper.audio.log_mel_spectrogram. */
int ccx_whisper_set_max_audio(ccx_whisper* w, double seconds);
/* Opt-in, before finalize (default off): keep a block-scaled FP8 image of the encoder output ("FP8 encoder-output stream" above) and
 * let the cross attention of decodes on the X-stream path (ccx_whisper_last_cross_path == 2) stream it instead of the bf16 rows: half
 * the bytes per element.  ccx_whisper_encode then ends with a quantise kernel that writes the image AND overwrites the instance's
 * bf16 encoder output with xhat, so every other consumer (the K / V projection of the <= 80-sequence paths, the alignment kernels,
 * xa_out_dev) sees the values the stream sees.  Refused (CCX_ERR_ARG, the message names the reason) when the instance has no X-stream
 * path: n_audio_state not a width csrc/cross_x.hip instantiates (128, 256, 384, 512, 768 -- so not the 1280-wide family), decoder and
 * encoder width different, or CCX_CROSS_X=0 in the environment.  Where this was not called, CCX_CROSS_FP8=1 in the environment at
 * ccx_whisper_finalize turns it on (ignored, not refused, on an instance without an X-stream path).  An instance with it off
 * allocates nothing more, runs no other kernel and computes the bits it always did.
 * CCX_XS_FP8=0 (read per call with the other chain switches, part of the step graphs' key): an FP8 instance streams its bf16 xhat
 * instead of the image -- the same bits, for A/B; no effect on a default instance.
 * What the quantisation costs in transcript quality on real checkpoints is NOT measured. */
int ccx_whisper_set_cross_fp8(ccx_whisper* w, int on);
/* 1 when the instance keeps and streams the FP8 image (after finalize: the environment switch included), else 0. */
int ccx_whisper_cross_fp8(ccx_whisper* w);
/* Opt-in, before finalize (default off): the reduced audio context ("audio_ctx" of other Whisper runtimes) -- the instance accepts
 * ccx_whisper_encode_ctx, which keeps only the first n_ctx[b] of the n_audio_ctx encoder positions of window b, and the cross attention
 * of every decode reads those n_ctx[b] rows only.  This is NOT upstream's arithmetic: Whisper was trained on zero-padded 30 s windows,
 * and what attending over fewer positions costs in transcript quality on real checkpoints is NOT measured.
 * The counts live in a device array of max_batch ints which the X-stream cross attention (csrc/cross_x.hip, XsParams::seq_S) reads;
 * it is the only cross attention with a count per sequence, so on such an instance EVERY decode entry point (decode, decode_greedy,
 * decode_rows, decode_beam, decoder_logits, detect_language; prefill and lanes included) takes the X-stream path at every batch size
 * (ccx_whisper_last_cross_path == 2), and the alignment pass runs its decoder rows on it as well.  Refused (CCX_ERR_ARG, the message
 * names the reason) under the rule of ccx_whisper_set_cross_fp8: no X-stream path (the 1280-wide family, unequal encoder / decoder
 * widths, CCX_CROSS_X=0).  An instance with it off allocates nothing more, launches what it always launched and computes the bits it
 * always did. */
int ccx_whisper_set_audio_ctx(ccx_whisper* w, int on);
/* 1 when the instance was built for the reduced audio context, else 0. */
int ccx_whisper_audio_ctx(ccx_whisper* w);
/* Optional, before finalize: take the log-mel / encoder workspaces of `donor` (finalized, same dimensions, at least this
 * instance's capacity) instead of allocating them.  They are only live between ccx_whisper_logmel / set_mel and the end of
 * ccx_whisper_encode.  Users of one group are ordered by the library: every logmel / set_mel waits (event) for the end of the
 * group's previous encode, on whatever streams they run -- so an instance may encode while ANOTHER instance of the group decodes
 * (the software-pipelined batch driver), but the host must issue logmel / set_mel .. encode of one instance as an UNINTERRUPTED pair:
 * the event orders a logmel behind the group's previous encode only, and between an instance's logmel and its encode the workspaces
 * hold its staged windows.  Enforced: a logmel / set_mel of another instance of the group in between fails with CCX_ERR_ARG.
 * A donor destroyed while takers are alive is freed when its last taker is destroyed. */
int ccx_whisper_share_encoder_scratch(ccx_whisper* w, ccx_whisper* donor);
/* Checks every tensor is present, builds the fused/bf16 device layouts, uploads. */
int ccx_whisper_finalize(ccx_whisper* w);
int ccx_whisper_set_rules(ccx_whisper* w, const ccx_decode_rules* rules);

/* Per-call decoding options (openai-whisper decoding.py::DecodingOptions without_timestamps, suppress_blank, suppress_tokens,
 * max_initial_timestamp [UPSTREAM-RECALL]; parity unpinned).  ccx_decode_options_default fills {0, 1, -2, 0, NULL}: the decode the
 * rules alone give.
 *   without_timestamps 1: the step ends in the select / beam kernels WITHOUT ApplyTimestampRules (their own instantiations): an id
 *     is allowed when the call's mask does not suppress it and, on the first sampled step with suppress_blank on, it is neither
 *     rules.blank nor rules.eot.  No text / timestamp ranges, no forced timestamp, no max_initial_timestamp; timestamp ids and
 *     <|notimestamps|> are not banned.  The caller's prompts end in <|notimestamps|>.
 *   suppress_blank: read by the kernels without the rules only -- with the rules the first step bans every text id and eot anyway.
 *   max_initial_timestamp_index: -2 the rules' own value, -1 the rule off, >= 0 this index (at most n_vocab - timestamp_begin - 1).
 *   suppress / n_suppress: NULL = the rules' list; otherwise the list that REPLACES it (host array, copied; n_suppress 0 with a
 *     non-NULL pointer: nothing is suppressed).  Every id must lie in [0, n_vocab).
 * ccx_whisper_set_decode_options is sticky like ccx_whisper_set_rules (NULL: back to the defaults) and checked like it: CCX_ERR_ARG
 * (1) naming "ccx_whisper_set_decode_options" and the field.  It needs the rules.  The instance keeps a SECOND device mask for the
 * options: the list above (or the rules'), <|notimestamps|> unless without_timestamps is set, and always the ids [n_vocab, n_vocab
 * rounded up to 4).  Whether a step reads that mask, without_timestamps, suppress_blank and the max_initial_timestamp index are part
 * of the step plan, so the captured graphs of default decodes and of option decodes live side by side; a call that changes the
 * mask's contents drops the graphs of the option plans only.  ccx_whisper_set_rules resets the options to the defaults.
 * ccx_whisper_decode, _decode_rows, _decode_beam and _decode_greedy honour them. */
typedef struct ccx_decode_options {
  int without_timestamps;
  int suppress_blank;
  int max_initial_timestamp_index;
  int n_suppress; const int* suppress;
} ccx_decode_options;
void ccx_decode_options_default(ccx_decode_options* opts);
int ccx_whisper_set_decode_options(ccx_whisper* w, const ccx_decode_options* opts);
/* Captured step graphs the instance holds (options_only != 0: those of option plans only); -1 for a NULL handle.  A test aid: a
 * default decode after an option decode must find its graph where it left it. */
int ccx_whisper_graph_count(ccx_whisper* w, int options_only);

/* The two per-call rules over a row's own sampled history: repetition_penalty and no_repeat_ngram_size, as CTranslate2 /
 * faster-whisper and Hugging Face name them (the rule is ours, in the form of HF's RepetitionPenaltyLogitsProcessor and
 * NoRepeatNGramLogitsProcessor; parity unpinned; restated in tests/history_rules_reference.py).  ccx_decode_history_options_default
 * fills {1.0f, 0}: both off.  For one row in the sampling phase, H = the m tokens THIS decode has sampled so far (not the prompt, the
 * SOT sequence or a prefix) and E = rules.eot; ids >= E -- eot, the specials, the timestamps -- are never edited, so the timestamp
 * rules and closed pairs <|t|><|t|> keep working:
 *   1. repetition_penalty p (finite, > 0; 1.0 = off): every distinct v in H with v < E: x = logits[v]; logits[v] = x > 0 ? x / p : x * p
 *      in fp32, once per id however often it occurs.
 *   2. no_repeat_ngram_size n (>= 0; 0 = off), only when m >= n: for every i in [0, m - n] with H[i : i+n-1] == H[m-n+1 : m] and
 *      H[i+n-1] < E: logits[H[i+n-1]] = -inf.  n = 1 bans every text id sampled so far; the matched context may hold ids >= E.
 *   1 comes before 2; both come BEFORE SuppressBlank, SuppressTokens, ApplyTimestampRules and the sampler (csrc/dec_history.hip:
 *   dec_history_kernel, one block per row, between the logits GEMM and the select / beam top-k kernel), so sum_logprob is taken from
 *   the edited logits, as HF does; no_speech_prob is untouched (it is read where H is empty).  Rows that are done or still in the
 *   prompt phase are not touched.  DEVIATION from HF, stated: HF penalises and bans over prompt + generated ids and exempts nothing.
 * ccx_whisper_set_history_options is sticky like ccx_whisper_set_decode_options (NULL: back to the defaults), needs the rules, and
 * is checked like it: CCX_ERR_ARG (1) naming "ccx_whisper_set_history_options" and the field for a repetition_penalty that is not
 * finite or <= 0 and a negative no_repeat_ngram_size (one above sample_len is legal and never fires).  ccx_whisper_set_rules resets
 * it.  Both values are part of the step plan: with {1.0, 0}, set or not, a decode takes the plan, the launches and the graphs it
 * always took; the graphs of history plans live beside those of default and option plans.  ccx_whisper_decode, _decode_greedy,
 * _decode_rows and _decode_beam (whose rows read the history that follows their hypothesis) honour the setting;
 * ccx_whisper_decoder_logits, _align and _align_probs do not: word probabilities stay those of the raw model. */
typedef struct ccx_decode_history_options {
  float repetition_penalty;
  int no_repeat_ngram_size;
} ccx_decode_history_options;
void ccx_decode_history_options_default(ccx_decode_history_options* opts);
int ccx_whisper_set_history_options(ccx_whisper* w, const ccx_decode_history_options* opts);
/* Captured step graphs of history plans the instance holds (a test aid, like ccx_whisper_graph_count); -1 for a NULL handle. */
int ccx_whisper_history_graph_count(ccx_whisper* w);

/* Vocabulary control per call: sequence_bias, and through it bad_words_ids and hotwords (the rule is ours, in the form of Hugging
 * Face's SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor; parity unpinned; restated in tests/bias_reference.py).  The
 * single-token suppress masks cannot express it: the bias on the last id of a phrase depends on what the row has just sampled.
 *   TABLE.  An ordered list of n_entries entries (ids[0 .. L), bias): entry e holds ids[offsets[e] .. offsets[e + 1]) and bias[e].
 *     1 <= L <= CCX_BIAS_MAX_LEN; every id in [0, n_vocab); the TARGET ids[L - 1] is < E = rules.eot (ids >= E -- eot, the specials,
 *     the timestamps -- are never edited, as with the history rules; context ids may be any id); bias is finite or -inf (+inf and NaN
 *     are refused).  bad_words_ids are entries with bias -inf.  At most CCX_BIAS_MAX_ENTRIES entries and CCX_BIAS_MAX_IDS ids.
 *   HISTORY.  For one row in the sampling phase, H = the m = n_gen ids THIS decode has sampled: the H of the history rules, without
 *     the prompt, the SOT sequence or a prefix; for beam rows the history that follows the hypothesis.
 *   TERMS.  b1[v] = the fp32 sum, in table order, of the length-1 entries with target v.  S[v] = the fp32 sum, in table order, of
 *     the entries with L >= 2, target v, L - 1 <= m and H[m - L + 1 : m] == ids[0 : L - 1].
 *   EDIT.  logits[v] = (logits[v] + b1[v]) + S[v] in fp32.  A term that does not exist is skipped, not added as zero; each term
 *     lands once per id.  Rows that are done or still in the prompt phase are not touched.
 *   ORDER.  The edit comes BEFORE the history rules (ccx_decode_history_options), the order of transformers' _get_logits_processor
 *     (sequence bias, repetition penalty, no-repeat n-gram; a -inf commutes with all of them), and so before SuppressBlank,
 *     SuppressTokens, ApplyTimestampRules, the temperature and the sampler; sum_logprob is taken from the edited logits.
 *   DEVIATION from HF, stated: HF matches over prompt + generated ids and exempts no id; and the installed processor skips an entry
 *     whose L ids outnumber its input_ids, so an entry whose context is the WHOLE history (L - 1 == m) never fires there; here it
 *     does (a bad bigram holds from the second sampled token on).
 *   CONSEQUENCE, stated: with length-1 entries the first sampled step's row is edited, and where no_speech_prob is read from that
 *     row (<|startoftranscript|> is the prompt's last token: no SOT tail, no prefix, n_vocab a multiple of 4) it is the softmax of the
 *     EDITED row.  Without a length-1 entry, and wherever it is read at an earlier prompt position, it is bit-identical to an unbiased
 *     decode's.
 * csrc/dec_bias.hip: dec_bias_kernel, one block per row between the logits GEMM and dec_history_kernel / the select / beam top-k
 * kernel; no atomics, so the sums' order and bits are fixed.  The table is compiled on the host (a stable sort: length-1 entries by
 * target, the others by (last context id, target), the caller's order kept inside a group) into fixed-capacity device buffers the
 * instance owns, allocated at the first non-empty table; the kernel reads every count from a small device header, so a captured
 * step graph serves every later table.
 * ccx_decode_bias_options_default fills zeros: off.  ccx_whisper_set_bias_options is sticky like ccx_whisper_set_history_options
 * (NULL or n_entries == 0: off), needs the rules, is reset by ccx_whisper_set_rules, and is checked on the host: CCX_ERR_ARG (1)
 * naming "ccx_whisper_set_bias_options" and the field for n_entries outside [0, CCX_BIAS_MAX_ENTRIES], NULL arrays, offsets that do
 * not start at 0 or do not ascend, an entry length outside [1, CCX_BIAS_MAX_LEN], more than CCX_BIAS_MAX_IDS ids, an id outside
 * [0, n_vocab), a target >= eot, a bias that is +inf or NaN, and length-1 entries of one target whose sum is.  All three arrays are
 * HOST memory and are copied.  One step-plan field says whether a table is set: with none, set or not, a decode takes the plan, the
 * launches and the graphs it always took; the graphs of bias plans live beside those of default, option and history plans.
 * ccx_whisper_decode, _decode_greedy, _decode_rows and _decode_beam honour the setting; ccx_whisper_decoder_logits, _align and
 * _align_probs do not. */
#define CCX_BIAS_MAX_ENTRIES 8192
#define CCX_BIAS_MAX_IDS 65536
#define CCX_BIAS_MAX_LEN 32
typedef struct ccx_decode_bias_options {
  int n_entries;
  const int* offsets;       /* HOST [n_entries + 1] */
  const int* ids;           /* HOST [offsets[n_entries]] */
  const float* bias;        /* HOST [n_entries] */
} ccx_decode_bias_options;
void ccx_decode_bias_options_default(ccx_decode_bias_options* opts);
int ccx_whisper_set_bias_options(ccx_whisper* w, const ccx_decode_bias_options* opts);
/* Captured step graphs of bias plans the instance holds (a test aid, like ccx_whisper_history_graph_count); -1 for a NULL handle. */
int ccx_whisper_bias_graph_count(ccx_whisper* w);

/* Truncated sampling per call: top_k, top_p and min_p, as Hugging Face `generate` names them (the rule is ours, in the form of HF's
 * TopKLogitsWarper, TopPLogitsWarper and MinPLogitsWarper applied after the temperature, in that order; parity unpinned; restated in
 * tests/truncation_reference.py).  ccx_decode_sampling_options_default fills {0, 1.0f, 0.0f}: all off.  For one row in the sampling
 * phase of a decode at temperature T > 0, x = the row after EVERY filter of the select kernel (SuppressTokens, SuppressBlank,
 * ApplyTimestampRules, and the ban on text ids where the timestamp mass forces a timestamp), A = {v : x_v > -inf}, p = softmax(x / T)
 * over A:
 *   1. top_k (>= 0; 0 = off): c1 = the k-th largest x over A, multiplicity counted (the minimum when |A| < k); keep x_v >= c1.  Ties
 *      at the k-th value all stay, as in HF.
 *   2. top_p (0 < top_p <= 1; 1 = off): over the survivors of 1, renormalised, keep v iff the mass of the survivors with x_u > x_v
 *      (strictly) is < top_p.  Without ties this is HF's removal of `cumulative_probs <= 1 - top_p`.  DEVIATION from HF, stated: of
 *      equal values HF keeps whichever its sort put last; here a tie is kept or dropped as a whole.
 *   3. min_p (0 <= min_p <= 1; 0 = off): keep v iff x_v >= x_max + T * ln(min_p), evaluated in fp32 as written (product and sum each
 *      rounded); HF's p_v >= min_p * p_max in logit space.
 *   All three keep an upper set of x, so K = {v : x_v >= cut} for one value cut; the maximum always survives.  The draw is the
 *   Gumbel-max of the untruncated sampler over the same Philox stream (seed, stream id, step, vocabulary id), restricted to K: a draw
 *   that lands in K is the draw an untruncated decode makes.  sum_logprob keeps its meaning, the unscaled log-softmax over the
 *   filtered UNTRUNCATED row; no_speech_prob is untouched; a row with A empty, a finished row and a row in its prompt phase behave as
 *   without truncation.  At T == 0 the three values have no effect.  The mass is exp2((x - max) * log2(e) / T) in fp32, summed in one
 *   fixed order without atomics (csrc/dec_truncate.h inside dec_select_kernel<SAMPLE, RULES, TRUNC = true>): the same row, seed and
 *   stream id give the same token in every launch geometry.
 * ccx_whisper_set_sampling_options is sticky like ccx_whisper_set_history_options (NULL: back to the defaults), needs the rules, is
 * reset by ccx_whisper_set_rules, and is checked: CCX_ERR_ARG (1) naming "ccx_whisper_set_sampling_options" and the field for
 * top_k < 0, top_p NaN or outside (0, 1], min_p NaN or outside [0, 1].  The three values live in device memory beside {temperature,
 * seed}, so a captured step graph serves every value; ONE step-plan field says whether truncation is on (any value off its default,
 * in a decode with T > 0): with {0, 1.0, 0.0}, set or not, a decode takes the plan, the launches and the graphs it always took.
 * ccx_whisper_decode and _decode_rows honour the setting on every cross-attention path and in every lane; ccx_whisper_decode_greedy
 * and _decode_beam ignore it. */
typedef struct ccx_decode_sampling_options {
  int top_k;
  float top_p;
  float min_p;
} ccx_decode_sampling_options;
void ccx_decode_sampling_options_default(ccx_decode_sampling_options* opts);
int ccx_whisper_set_sampling_options(ccx_whisper* w, const ccx_decode_sampling_options* opts);
/* Captured step graphs of truncation plans the instance holds (a test aid, like ccx_whisper_history_graph_count); -1 for a NULL handle. */
int ccx_whisper_sampling_graph_count(ccx_whisper* w);

/* Per-token log-probabilities and top-N alternatives (opt-in: ccx_whisper_set_token_logprobs before finalize, then
 * ccx_whisper_set_logprob_options per call; the rule is ours, parity unpinned; restated in tests/logprobs_reference.py).
 * Take a row that samples at this step (not in its prompt phase, not done).  x = its logit row as the step draws from it: after the
 * bias kernel, the history kernel, the suppress mask of the rules or the call's options, SuppressBlank, ApplyTimestampRules on ruled
 * plans, and the removal of the text ids when the summed timestamp mass beats the best text token.  x is NOT divided by the
 * temperature, NOT truncated by top_k / top_p / min_p, and carries no noise: it is the row sum_logprob is defined over.
 * A = {v : x_v > -inf}; lp_v = (x_v - mx_all) - lnorm in fp32, mx_all the maximum over A and lnorm = log sum_A exp(x - mx_all), as the
 * select kernel forms the chosen token's value (csrc/dec_head_row.h).
 *   token_logprob[step] is the float the kernel adds to sum_logprob at that step, bit for bit (whatever that is for a row with A
 *     empty).  One entry per sampled step; the step that samples eot has one; a finished row writes none.
 *   top[step][k], k < top_n, is (id, lp_id) of the top_n largest x_v over A in descending order; of equal values the lower id comes
 *     first (torch.argmax on the CPU); where |A| < top_n the rest is (-1, -inf).
 *   top_n lies in [0, CCX_LOGPROB_MAX_TOP]; 0 gives the chosen token's log-probability only.
 * So: at temperature 0 top[step][0] is the chosen token and its lp equals token_logprob[step] bit for bit; whenever the chosen id is
 * listed its lp there equals token_logprob[step] bit for bit; and the fp32 sum of a row's token_logprob entries, added in step order
 * from 0.0f, equals the returned sum_logprob bit for bit.
 * ccx_whisper_set_token_logprobs(w, 1) (before finalize) makes finalize allocate the three buffers beside the token histories:
 * [max_batch][n_text_ctx] floats and [max_batch][n_text_ctx][8] ids and floats; without it nothing more is allocated.
 * ccx_whisper_set_logprob_options is sticky like ccx_whisper_set_sampling_options (NULL: off), needs the rules, is reset by
 * ccx_whisper_set_rules, and is refused with CCX_ERR_ARG (1) naming "ccx_whisper_set_logprob_options" and the field when the instance
 * lacks the buffers or top_n lies outside [0, 8].  WHERE top_n LIVES: in the step plan -- its one new field is 0 with the setting
 * off and 1 + top_n with it on -- so the select kernel gets top_n as a launch parameter and a first decode with another top_n
 * captures exactly ONE more step graph per lane plan (ccx_whisper_logprob_graph_count); with the setting off, set or not, a decode
 * takes the plan, the launches and the graphs it always took.  The buffers keep their addresses and a row's step index is its own
 * state, so the captured graphs stay valid across decodes.
 * ccx_whisper_decode and _decode_rows honour the setting at any temperature, on every cross-attention path and in every lane;
 * ccx_whisper_decode_greedy and _decode_beam ignore it (a beam's rows are rewritten by parent every step).
 * ccx_whisper_token_logprobs copies the values of the LAST decode to host arrays: tok_lp_out [R][sample_len], and, top_n > 0,
 * top_id_out / top_lp_out [R][sample_len][top_n] (top_n <= the decode's; NULL with top_n == 0).  R and sample_len are the decode's.
 * Entries at or beyond a row's sampled steps are NaN, -1 and -inf: the library fills the buffers when a recording decode starts.
 * Refused (CCX_ERR_STATE) when the last decode did not record them. */
#define CCX_LOGPROB_MAX_TOP 8
typedef struct ccx_decode_logprob_options {
  int top_n;
} ccx_decode_logprob_options;
int ccx_whisper_set_token_logprobs(ccx_whisper* w, int on);
int ccx_whisper_set_logprob_options(ccx_whisper* w, const ccx_decode_logprob_options* opts);
int ccx_whisper_token_logprobs(ccx_whisper* w, int R, int sample_len, float* tok_lp_out, int top_n, int32_t* top_id_out, float* top_lp_out,
                               void* stream);
/* Captured step graphs of log-probability plans the instance holds (a test aid, like ccx_whisper_history_graph_count); -1 for a NULL
 * handle. */
int ccx_whisper_logprob_graph_count(ccx_whisper* w);

/* Log-mel of B clips (whisper.audio.log_mel_spectrogram + pad_or_trim to 3000 frames).
 * audio_dev: [B, stride] f32; n_samples / seek_frames: host int arrays (seek may be NULL = 0).
 * Fills the model's conv-stem input; if mel_out_dev != NULL also writes [B, n_mels, 3000] f32. */
int ccx_whisper_logmel(ccx_whisper* w, const float* audio_dev, int64_t stride, const int* n_samples,
                       const int* seek_frames, int B, float* mel_out_dev, void* stream);
/* ccx_whisper_logmel with a cap on every window's frames (transcribe.py's clip_timestamps [UPSTREAM-RECALL]: a window ends where its
 * clip ends): max_frames host [B] (>= 0) or NULL; window b holds min(3000, content_frames - seek, max_frames[b]) frames of the clip's
 * log-mel and literal zeros behind them -- pad_or_trim of the cropped mel.  Still normalised by the WHOLE clip's maximum.
 * ccx_whisper_logmel is the NULL case. */
int ccx_whisper_logmel_ex(ccx_whisper* w, const float* audio_dev, int64_t stride, const int* n_samples, const int* seek_frames,
                          const int* max_frames, int B, float* mel_out_dev, void* stream);
/* Alternative input: take a ready [B, n_mels, 3000] f32 mel (BASELINE config 2 "mel [8,80,3000]"). */
int ccx_whisper_set_mel(ccx_whisper* w, const float* mel_dev, int B, void* stream);
/* AudioEncoder.forward for the B staged windows.  The encoder output (bf16) stays with the instance: decodes of more than 80 sequences
 * read it directly in their cross attention (csrc/cross_x.hip), decodes of <= 80 sequences project the per-layer cross-attention K / V
 * of their sequences out of it when they start (with CCX_CROSS_X=0 at ccx_whisper_finalize this call projects K / V for all B, as in
 * openai-whisper's kv_cache hooks).
 * xa_out_dev (optional): [B, n_audio_ctx, n_audio_state] f32 copy of the encoder output.  On an FP8 instance
 * (ccx_whisper_set_cross_fp8) it is xhat, the dequantised encoder output that the instance keeps and every decode reads. */
int ccx_whisper_encode(ccx_whisper* w, int B, float* xa_out_dev, void* stream);
/* The same at a reduced audio context (ccx_whisper_set_audio_ctx instances only): n_ctx host [B], every value in [64, n_audio_ctx].
 * The conv stem runs on the usual 3000-frame log-mel; positions [0, n_ctx[b]) of window b are kept, with rows [0, n_ctx[b]) of the
 * positional embedding; every encoder layer attends over those positions only; then ln_post.  The call runs S_run = max(n_ctx) rows (rounded
 * up to a multiple of 4) per sequence through the GEMMs and LayerNorms, and the attention takes the count per sequence (csrc/attention.hip, n_keys): rows of
 * a sequence between n_ctx[b] and S_run are computed and never read as keys, so a window's valid rows are, bit for bit, those of the
 * window encoded alone.  All n_ctx[b] == n_audio_ctx: the bits of ccx_whisper_encode.
 * The encoder output keeps its slot stride of n_audio_ctx rows per window (lane offsets, row maps, the FP8 image's stride and
 * captured step graphs stay valid), and the counts stay with the instance until the next encode: a plain ccx_whisper_encode resets
 * them to n_audio_ctx.  xa_out_dev (optional) is [B, n_audio_ctx, n_audio_state]; its rows at or beyond n_ctx[b] are unspecified.
 * ccx_whisper_align* after such an encode refuses a window whose n_frames / 2 exceeds its n_ctx. */
int ccx_whisper_encode_ctx(ccx_whisper* w, int B, const int* n_ctx, float* xa_out_dev, void* stream);

/* Teacher-forced decoder pass for parity tests: tokens [B, T] (host int32) -> logits
 * [B, T, n_vocab] f32 on device.  Uses the same step kernels as greedy decoding. */
int ccx_whisper_decoder_logits(ccx_whisper* w, const int32_t* tokens, int B, int T, float* logits_dev,
                               void* stream);

/* Greedy (temperature 0) DecodingTask.run for the B encoded windows.
 * prompt_ids: host [B, max_prompt] initial tokens (sot_prev + prompt + sot), prompt_lens: [B].
 * Outputs (host): tokens [B, sample_len] sampled ids (eot-padded), n_tokens [B] count before eot,
 * sum_logprob [B], no_speech_prob [B]. */
int ccx_whisper_decode_greedy(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens,
                              int max_prompt, int B, int sample_len, int32_t* tokens_out,
                              int32_t* n_tokens_out, float* sum_logprob_out, float* no_speech_prob_out,
                              void* stream);

/* DecodingTask.run with GreedyDecoder.update's temperature branch: temperature 0 = argmax (identical to
 * ccx_whisper_decode_greedy); temperature > 0 = one sample per step from Categorical(logits / temperature) over the
 * filtered logits -- what the reference gets from transcribe(..., temperature=self.config.temperature) with
 * Config.temperature = 0.1 (back/api.py:128, 1286-1292).  The draw is Gumbel-max over Philox4x32-10 noise keyed by
 * (seed, sequence row, step, vocabulary id): reproducible, independent of batch composition, but not bit-equal to
 * torch's sampler (distributional parity).  sum_logprob uses the unscaled log-softmax, as upstream. */
int ccx_whisper_decode(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int B,
                       int sample_len, float temperature, uint64_t seed, int32_t* tokens_out, int32_t* n_tokens_out,
                       float* sum_logprob_out, float* no_speech_prob_out, void* stream);

/* ccx_whisper_decode for R <= max_batch rows over the n_windows <= max_batch windows of the last ccx_whisper_encode: row r keeps
 * self-attention cache slot r and its cross attention reads window window_of_row[r] (host [R]; entries may repeat, need not be
 * monotone, and windows may go unused).  What openai-whisper's transcribe.py::decode_with_fallback [UPSTREAM-RECALL] needs when it decodes
 * a window again at the next temperature -- only the failing windows, nothing encoded again -- and what DecodingOptions.best_of needs
 * (decoding.py: `audio_features.repeat_interleave(self.n_group, dim=0)`): n rows on one window without copies of its encoder output.
 * stream_ids (host [R], >= 0, or NULL = the row index): the sampler's noise stream of every row, so that a row's draws do not depend
 * on which other rows share the call.  The cross-attention path is chosen by R as ccx_whisper_decode chooses it by B; the per-layer
 * K/V are projected for n_windows (an X-stream instance whose K/V caches cannot hold n_windows takes the X-stream path).  <= 16 rows
 * at d_model 768 run the two-launch query instead of the fused one (bit-identical q).  Everything ccx_whisper_decode checks is
 * checked, plus the ranges above: CCX_ERR_ARG (1) naming "ccx_whisper_decode_rows" and the field.  Outputs as ccx_whisper_decode. */
int ccx_whisper_decode_rows(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int R,
                            const int32_t* window_of_row, int n_windows, const int32_t* stream_ids, int sample_len, float temperature,
                            uint64_t seed, int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out,
                            float* no_speech_prob_out, void* stream);

/* Beam search (decoding.py::BeamSearchDecoder + DecodingTask._main_loop [UPSTREAM-RECALL]; parity unpinned) at temperature 0 for G
 * groups of beam_size consecutive rows over the n_windows windows of the last ccx_whisper_encode: group g decodes window
 * window_of_group[g] (host [G]; NULL: group g reads window g, G <= n_windows), its rows share that window's encoder output or K/V
 * through the row -> window map of ccx_whisper_decode_rows, so nothing is copied.  prompt_ids host [G][max_prompt], prompt_lens [G]:
 * one prompt per group (every row prefills it into its own cache slot).  Each step: logits GEMM, then dec_beam_topk_kernel and
 * dec_beam_update_kernel (csrc/dec_beam.hip) instead of the select kernel; the self attention reads its keys through a cache
 * indirection (uint16 [max_batch][n_text_ctx], allocated by the first beam decode) that follows a hypothesis when it moves to another
 * row -- no cache is copied or doubled.  A group is complete when it holds max_candidates finished hypotheses (round(beam_size *
 * patience)) and freezes; the call ends when all are, or at sample_len.  A group with fewer than beam_size finished hypotheses is
 * topped up with its live rows by descending score.  A beam decode runs in ONE lane whatever its row count; it takes the prefill
 * (CCX_PREFILL=0 is refused) and the step graphs, keyed by beam_size and max_candidates too.
 * Outputs (host), C = max(beam_size, max_candidates): tokens_out [G][C][sample_len] (tokens before the eot, eot-padded), n_tokens_out
 * / sum_logprob_out [G][C], n_hyp_out [G] (hypotheses of group g, in insertion order: finished ones first), no_speech_prob_out [G].
 * trace (NULL: off; a test aid -- a traced decode runs its steps eagerly): host buffers, n_steps rows of R = G * beam_size entries,
 * that receive per sampled step and row the proposals (cand_id / cand_lp [n_steps][R][beam_size + 1]), the chosen token, the row it
 * continues and its cumulative score (tok / parent / score [n_steps][R]); entries of steps a group no longer took stay -1 / NaN.
 * Checks everything ccx_whisper_decode_rows checks, plus 1 <= beam_size <= 8, 1 <= max_candidates <= 16, G * beam_size <= max_batch:
 * CCX_ERR_ARG (1) naming "ccx_whisper_decode_beam" and the field. */
typedef struct ccx_beam_trace {
  int n_steps;
  int32_t* cand_id; float* cand_lp; int32_t* tok; int32_t* parent; float* score;
} ccx_beam_trace;
int ccx_whisper_decode_beam(ccx_whisper* w, const int32_t* prompt_ids, const int32_t* prompt_lens, int max_prompt, int G,
                            const int32_t* window_of_group, int n_windows, int beam_size, int max_candidates, int sample_len,
                            int32_t* tokens_out, int32_t* n_tokens_out, float* sum_logprob_out, int32_t* n_hyp_out,
                            float* no_speech_prob_out, const ccx_beam_trace* trace, void* stream);

/* ---- the decode step's attention and token-select kernels on their own (csrc/decoder.hip; for kernel parity tests) ---------
 * Both entry points check on the host everything the kernels assume (ranges, element counts, 16-byte alignment of every
 * vector-accessed pointer) before anything is launched: a violation returns CCX_ERR_ARG (1) with a message naming the field.
 * They own their scratch, free it on every path and synchronise the stream. */
#define CCX_DEC_ATTN_SELF 0          /* dec_attention_kernel<true>: keys [0, pos[row]] */
#define CCX_DEC_ATTN_SPLIT 1         /* dec_attention_kernel<false> (nsplit partials), then dec_combine_kernel if `combine` */
#define CCX_DEC_ATTN_STREAM 2        /* stream_mode = 1: dec_cross_stream_kernel<true, NP>; T > 1536 falls back to dec_attention_kernel<true> */
#define CCX_DEC_ATTN_PREFILL 3       /* rows_per_seq == 2: dec_cross_stream_kernel<.., true>; >= 3: dec_cross_prefill_kernel<NP, 4> */
#define CCX_DEC_ATTN_FUSED_Q 4       /* ccx_launch_dec_cross_fused_q: q = LN(x + pending slabs) Wq^T + bq inside the attention blocks */
#define CCX_DEC_ATTN_TWO_LAUNCH_Q 5  /* dec_linear<ACT_LN, DEPI_F32>, then dec_attention_kernel<false>: what FUSED_Q replaces */
/* (6 is not a form: it stays the number the rejection tests of the descriptor use for an unknown one) */
#define CCX_DEC_ATTN_STREAM_MAPPED 7 /* form 2 with row_seq honoured: dec_cross_stream_kernel<true, NP, false, true> (ccx_whisper_decode_rows) */
#define CCX_DEC_ATTN_SELF_IND 8      /* form 0 through a cache indirection: dec_attention_kernel<true, true> (ccx_whisper_decode_beam) */

typedef struct ccx_dec_attn_desc {
  /* device operands.  q f32 [rows][H][64] (forms 0..3, 7, 8); k, v bf16 [n_seq][H][kv_T][64] */
  const void* q; const void* k; const void* v;
  int rows, n_seq, H, kv_T;
  int T;                    /* keys [0, T) of the cross forms (1..5, 7) */
  const int* pos;           /* HOST [rows], forms 0, 8: row r attends to keys [0, pos[r]] */
  const int* row_seq;       /* HOST [rows] or NULL (row r reads sequence r): forms 0, 1, 3, 7 */
  int rows_per_seq;         /* form 3: consecutive groups of that many rows belong to one sequence (group g = sequence g) */
  int nsplit, combine;      /* forms 1, 4, 5: key splits (1..8); form 1: also run dec_combine_kernel into out */
  int lds_pad;              /* forms 1, 2, 7: dynamic LDS the blocks claim without using it */
  /* forms 4, 5 (H must be 12): x f32 [rows][768], pend f32 [max(pend_n, 1)] slabs of [rows][768] pend_stride elements apart (slab 0
   * is read, with weight 0, also when pend_n == 0), ln_g / ln_b / bq f32 [768] on the device, wq f32 [768][768] row-major on the HOST */
  const void* x; const void* pend; int pend_n; int64_t pend_stride;
  const void* ln_g; const void* ln_b; float eps;
  const float* wq_host; const void* bq;
  /* device outputs: out f32 [rows][H * 64] (the kernels' bf16 output widened; forms 0, 2, 3, 7, 8 and form 1 with combine),
   * part_o f32 [rows][H][nsplit][64], part_ml f32 [rows][H][nsplit][2] (forms 1, 4, 5), q_x_out f32 [rows][768] (forms 4, 5, may be NULL) */
  void* out; void* part_o; void* part_ml; void* q_x_out;
  /* elements (of the buffer's own type) behind each pointer; kv_elems holds for k and for v */
  int64_t q_elems, kv_elems, out_elems, part_o_elems, part_ml_elems, x_elems, pend_elems, q_x_out_elems;
  /* form 8: HOST [rows][ind_ld], ind_ld > every pos[r]: key t <= pos[r] of row r is read from sequence ind[r * ind_ld + t], which must
   * lie in [0, n_seq); row_seq must be NULL.  (Appended: the forms before it read nothing here.) */
  const uint16_t* ind; int ind_ld;
} ccx_dec_attn_desc;

/* Fills a DecAttnParams and calls the production launchers unchanged (ccx_launch_dec_attention, ccx_launch_dec_combine,
 * ccx_launch_dec_cross_fused_q, ccx_launch_dec_linear).  Softmax scale 1/8.  With the profile on (ccx_prof_enable) the records name
 * the instantiation that ran. */
int ccx_dec_attention_desc(ccx_ctx* ctx, int form, const ccx_dec_attn_desc* desc, void* stream);

/* Per-sequence state of the select kernel (csrc/decoder.h DecSeqState, field for field). */
typedef struct ccx_dec_seq_state {
  int pos, prompt_len, n_gen, done;
  int last_tok, pen_tok, last_ts_tok, n_tokens;
  float sum_logprob, no_speech_prob;
} ccx_dec_seq_state;

typedef struct ccx_dec_select_desc {
  const void* logits; int64_t ld; int n_vocab; int B;   /* device f32 [B][ld] */
  const ccx_decode_rules* rules;                        /* the suppress mask is built as ccx_whisper_set_rules builds it */
  ccx_dec_seq_state* state;                             /* HOST [B], in and out */
  const int* prompt; int max_prompt;                    /* HOST [B][max_prompt] */
  int sample_len;
  int* gen;                                             /* HOST [B][sample_len], in and out */
  int* cur_tok; int* pos;                               /* HOST [B], in and out */
  int* n_done;                                          /* HOST [1], in and out */
  const void* tok_emb; const void* pos_emb; void* x; int D;   /* device f32 [tok rows][D], [pos rows][D], [B][D] (in and out) */
  int sample; float temperature; uint64_t seed; int row0;     /* sample 1: the kernel with the temperature > 0 branch */
  int64_t logits_elems, tok_emb_elems, pos_emb_elems, x_elems;
  const int* stream_ids;                                      /* HOST [B] (>= 0) or NULL: the noise stream of row b instead of row0 + b */
  const ccx_decode_options* opts;                             /* NULL: the rules alone (appended: nothing before it moves) */
  /* truncated sampling (appended: nothing before it moves).  sampling != NULL launches the truncating instantiation (needs sample = 1;
   * checked as ccx_whisper_set_sampling_options checks it), whatever the three values are.  cut_out / kept_out / kept_mass_out: HOST
   * [B] or NULL, written only for rows that sampled in this launch (temperature > 0, not done, not in the prompt phase): the smallest
   * kept logit (-inf for a row with nothing allowed), |K|, and the mass of K under softmax(x / T).  They need `sampling`. */
  const ccx_decode_sampling_options* sampling;
  float* cut_out; int* kept_out; float* kept_mass_out;
  /* per-token log-probabilities (appended: nothing before it moves).  logprobs != NULL launches the LOGP instantiation (top_n checked
   * as ccx_whisper_set_logprob_options checks it).  HOST outputs, in and out, written only for rows that sampled in this launch:
   * tok_logprob_out [B] (required), top_id_out / top_lp_out [B][top_n] (required when top_n > 0, not read when it is 0).  The
   * outputs need `logprobs`. */
  const ccx_decode_logprob_options* logprobs;
  float* tok_logprob_out; int* top_id_out; float* top_lp_out;
} ccx_dec_select_desc;

/* One launch of the select kernel (ccx_launch_dec_select) for B rows: filters, argmax / sampling, the per-sequence state machine and
 * the next step's embedding x[b] = tok_emb[next] + pos_emb[pos]. */
int ccx_dec_select_step(ccx_ctx* ctx, const ccx_dec_select_desc* desc, void* stream);

/* The > 16-row decode chain's LayerNorm -> linear pairs on their own (csrc/decoder.hip; for kernel parity tests): the production
 * launchers unchanged, dec_resolve_ln_kernel (no pending slabs) into bf16 rows, then
 *   F == 0:  dec_linear<ACT_BF16, epi>(W [N][K]) on those rows;
 *   F  > 0:  dec_linear<ACT_BF16, GELU>(W1 [F][K]) into bf16 rows [M][F], then dec_linear<ACT_BF16, epi>(W [N][F]) on those.
 * packed = 1 passes every bf16 row buffer between two kernels as the fragment image (csrc/decoder.h dec_frag_off), 0 row-major; the
 * buffers hold whole 16-row tiles and start out as NaN bit patterns, as does `out`.  epi and what `out` (device f32) receives:
 *   CCX_DEC_EPI_PARTIAL   [ksplit][M][N], the split-K slabs (ksplit = 1 up to 1024 input columns, 3 at 3072)
 *   CCX_DEC_EPI_F32       [M][N]
 *   CCX_DEC_EPI_SELF_QKV  [3][M][K]: q, then the k and v rows the epilogue appended to a one-position cache (N == 3 K, F == 0)
 *   CCX_DEC_EPI_GELU      [M][N]: the bf16 rows widened, read back through the layout they were written in
 * Checked on the host, CCX_ERR_ARG (1) naming "ccx_dec_ln_linear" and the field: 1 <= M <= 4096; K a multiple of 32 (64 for SELF_QKV)
 * in [128, 1280] but 160, 192 and 288; F 0 or a multiple of 32 up to 5120 -- K, and F where given, must leave no K slice of 1, 2, 3,
 * 5, 6 or 9 k-steps of 32 columns, in which one of a block's 4 waves would own none (ccx_launch_dec_linear refuses them); N a multiple of 4 (32 for GELU) up to 8192; 16-byte alignment and the element
 * counts.  x f32 [M][K], ln_g / ln_b f32 [K], b1 f32 [F], bias f32 [N] on the device; w1 f32 [F][K] and w f32 [N][K or F] row-major
 * on the HOST.  Owns its scratch; synchronises the stream. */
#define CCX_DEC_EPI_PARTIAL 0
#define CCX_DEC_EPI_F32 1
#define CCX_DEC_EPI_SELF_QKV 2
#define CCX_DEC_EPI_GELU 3
typedef struct ccx_dec_ln_linear_desc {
  int M, K, F, N, epi, packed;
  const void* x; const void* ln_g; const void* ln_b; float eps;
  const float* w1_host; const void* b1;
  const float* w_host; const void* bias;
  void* out;
  int64_t x_elems, out_elems;
} ccx_dec_ln_linear_desc;
int ccx_dec_ln_linear(ccx_ctx* ctx, const ccx_dec_ln_linear_desc* desc, void* stream);

/* ONE launch of dec_linear_kernel on its own (csrc/decoder.hip; for kernel parity tests; the product path does not call it): the
 * parameter block filled as the decode step fills it (whisper.hip dec_step: ln_linear, partial_linear) and ccx_launch_dec_linear
 * unchanged.  act picks the prologue, epi (CCX_DEC_EPI_*) the epilogue; the pairs the launcher has are LN with F32, SELF_QKV and GELU,
 * COMBINE with PARTIAL, and BF16 with all four.  out[M][N] = act[M][K] W[N][K]^T + bias, W rounded to bf16.
 *   CCX_DEC_ACT_LN       act = bf16(LayerNorm(x + pend[0] + .. + pend[pend_n - 1])): x f32 [M][K]; pend f32 slabs of [M][K] pend_stride
 *                        elements apart, added in fp32 one after the other.  Slab 0 is READ ALSO WHEN pend_n == 0 (with weight 0):
 *                        it must be readable and finite then.  x_out (or NULL) receives the resolved rows, ln_mean_out (or NULL) [M]
 *                        every row's centring shift: its mean where |mean| exceeds its std, else 0.  ln_g / ln_b f32 [K].
 *   CCX_DEC_ACT_BF16     act_rows bf16 [M][lda] row-major.
 *   CCX_DEC_ACT_COMBINE  act = bf16(merge of the split-KV partials part_o f32 [M][K / 64][nsplit][64], part_ml f32 [..][nsplit][2]).
 * What `out` receives:
 *   CCX_DEC_EPI_F32       f32 [M][ldo]
 *   CCX_DEC_EPI_GELU      bf16 [M][ldo]: erf-GELU of the sums
 *   CCX_DEC_EPI_PARTIAL   f32 [ksplit][M][ldo], the slabs out_stride elements apart; ksplit = ceil(K / 1024), or ceil(K / 1280) where that
 *                         exceeds 4; slab z sums the k-steps [z per_z, (z + 1) per_z), per_z = ceil(K / 32 / ksplit); the bias is in slab 0
 *   CCX_DEC_EPI_SELF_QKV  N == 3 K: q f32 [M][K] (the epilogue does not read ldo) and the k / v rows as bf16 into cache_k / cache_v
 *                         [n_seq][K / 64][cache_T][64] at (row_seq[m] or m, head, pos[m]); pos and row_seq are HOST [M]
 * Every device buffer is the caller's, in its own type, and nothing else of it is written.  Checked on the host before any launch,
 * CCX_ERR_ARG (1) naming "ccx_dec_linear_op" and the field: the pair; 1 <= M <= 16 for LN and COMBINE (the product's range), <= 4096
 * for BF16; K a multiple of 32 (64 for COMBINE and SELF_QKV), <= 1280 for LN and COMBINE, and such that no K slice leaves a wave
 * without a k-step (a slice of 1, 2, 3, 5, 6 or 9 k-steps of 32 columns: K = 32, 64, 96, 160, 192, 288); at most 4 slabs, and one
 * unless PARTIAL; N a multiple of 4; ldo >= N (K for SELF_QKV) and a multiple of 4; lda >= K and a multiple of 8; 0 <= pend_n <= 4;
 * pend_stride >= M K and a multiple of 4; x_out != x; 1 <= nsplit <= 8; out_stride >= M ldo and a multiple of 4; 0 <= pos[m] <
 * cache_T, 0 <= row_seq[m] < n_seq (M <= n_seq without row_seq), no (sequence, pos) named twice; 16-byte alignment of every device
 * pointer but ln_mean_out; every extent within its element count (of the buffer's own type).  Owns the packed weights and the two
 * index arrays only; synchronises the stream. */
#define CCX_DEC_ACT_LN 0
#define CCX_DEC_ACT_BF16 1
#define CCX_DEC_ACT_COMBINE 2
typedef struct ccx_dec_linear_desc {
  int act, epi, M, N, K;
  const float* w_host;                                  /* HOST f32 [N][K] row-major */
  const void* bias;                                     /* device f32 [N] or NULL */
  const void* x; const void* pend; int pend_n; int64_t pend_stride; void* x_out;       /* ACT_LN */
  const void* ln_g; const void* ln_b; float eps; void* ln_mean_out;
  const void* act_rows; int64_t lda;                    /* ACT_BF16 */
  const void* part_o; const void* part_ml; int nsplit;  /* ACT_COMBINE */
  void* out; int64_t ldo; int64_t out_stride;           /* out_stride: PARTIAL only */
  void* cache_k; void* cache_v; int cache_T, n_seq;     /* SELF_QKV */
  const int* pos; const int* row_seq;                   /* HOST [M]; row_seq may be NULL (row m is sequence m) */
  /* elements behind each pointer; ln_elems holds for ln_g and ln_b, cache_elems for cache_k and cache_v */
  int64_t bias_elems, x_elems, pend_elems, x_out_elems, ln_elems, ln_mean_out_elems, act_elems, part_o_elems, part_ml_elems,
      out_elems, cache_elems;
} ccx_dec_linear_desc;
int ccx_dec_linear_op(ccx_ctx* ctx, const ccx_dec_linear_desc* desc, void* stream);

/* The middle of a decode step's layer on the X-stream path, from the self attention to the cross-attention out projection, on its own
 * (for kernel parity tests): the production launchers unchanged, in the model's order --
 *   self attention (q, the self K/V cache, pos)                      -> attention rows (bf16)
 *   out projection Wo with the in-place residual resolve             -> x, its centred bf16 copy xb, xb's 16-column tile statistics
 *   LayerNorm-free cross-attention query + per-head expansion        -> xq (bf16)
 *   the streaming kernel over xa, then merge + value projection      -> attention rows (bf16)
 *   cross-attention out projection Wco, split-K partial epilogue     -> one f32 slab
 * packed = 1 asks for the bf16 rows between the kernels (both attention outputs, xb) as fragment images (csrc/decoder.h dec_frag_off); the
 * launcher takes them under the model's rule only (more than 16 rows, a multiple of 16) and reports what it took in *packed_used.
 * Inputs.  Device: q f32 [M][D]; self_k / self_v bf16 [M][H][kv_T][64]; x f32 [M][D]; shift f32 [M] or NULL (the rows' centring
 * shifts); xa bf16 [M][S][D] (row r attends to sequence r).  HOST: pos int [M] (row r attends to keys 0 .. pos[r]); row-major f32
 * weights wo, cq_w, ck_w, cv_w, co_w [D][D] and vectors bo, lnc_g, lnc_b, cq_b, cv_b, co_b [D], packed and folded inside as the model
 * does at finalize.
 * Output.  out, device f32, the parts back to back, every bf16 part widened and read back through the layout it was written in:
 *   attn_self [M][D] | x [M][D] | xb [M][D] | xb_stats [M][D / 16][2] | xq [M][H][D] | attn_cross [M][D] | co [M][D]
 * (ccx_dec_mid_chain_out_elems).  The scratch buffers hold whole 16-row tiles and start out as NaN bit patterns, as does `out`.
 * Checked on the host, CCX_ERR_ARG (1) naming "ccx_dec_mid_chain" and the field: 1 <= M <= 4096; H in {2, 4, 6, 8, 12} and D == 64 H
 * (the widths the X-stream kernels are instantiated for); 16 <= S <= 4096; 1 <= kv_T <= 4096 and 0 <= pos[r] < kv_T; packed 0 or 1;
 * non-NULL pointers, 16-byte alignment of the device ones, and the element counts.  Owns its scratch; synchronises the stream. */
typedef struct ccx_dec_mid_chain_desc {
  int M, D, H, S, kv_T, packed;
  const void* q; const void* self_k; const void* self_v; const void* x; const void* shift; const void* xa;
  const int* pos;
  const float* wo; const float* bo;
  const float* lnc_g; const float* lnc_b; const float* cq_w; const float* cq_b;
  const float* ck_w; const float* cv_w; const float* cv_b;
  const float* co_w; const float* co_b;
  void* out;
  int* packed_used;                                     /* HOST [1], out */
  int64_t q_elems, kv_elems, x_elems, xa_elems, out_elems;
} ccx_dec_mid_chain_desc;
int64_t ccx_dec_mid_chain_out_elems(int M, int D, int H);
int ccx_dec_mid_chain(ccx_ctx* ctx, const ccx_dec_mid_chain_desc* desc, void* stream);

/* One beam-search step on its own (csrc/dec_beam.hip: dec_beam_topk_kernel, one block per row, then dec_beam_update_kernel, one block
 * per window; the rule is restated in tests/beam_reference.py) for G windows of beam_size consecutive rows, R = G * beam_size.
 * Every row must be in the sampling phase (pos == prompt_len - 1 + n_gen); the rows of a window share n_gen, pos and done (a window
 * whose rows are done is complete: nothing of it is touched).  Tables, all HOST, in and out unless marked:
 *   state [R], hist [R][sample_len] (the tokens sampled so far first), cur_tok / pos [R], n_done [1] (+ beam_size per window that
 *   completes or runs out of its sample_len budget), ind uint16 [R][ind_ld] (the cache slots of every row's keys; ind_ld > pos + 1),
 *   fin_tok [G][max_candidates][sample_len] / fin_score / fin_n [G][max_candidates] / fin_count [G] (finished hypotheses: tokens before
 *   the eot, cumulative log-probability, token count; appended in descending score while a window holds fewer than max_candidates)
 *   out only: cand_id / cand_lp [R][beam_size + 1] (the proposals; id -1 where a row proposes nothing), tok_out / parent_out [R] (the
 *   chosen token and the row it continues; -1 for a window that did not step)
 * Device: logits f32 [R][ld], tok_emb, pos_emb, x f32 [R][D] (in and out).  Checked on the host before any launch, CCX_ERR_ARG (1)
 * naming "ccx_dec_beam_step" and the field: 1 <= G, R <= 65536, 1 <= beam_size <= 8, 1 <= max_candidates <= 16, n_vocab a multiple of 4
 * up to 53248, ld >= n_vocab and a multiple of 4, 16-byte alignment of every vector-accessed pointer, the element counts, every
 * state, ind entries of a live window < 65536, fin_count <= max_candidates.  Owns its scratch; synchronises the stream. */
typedef struct ccx_dec_beam_desc {
  const void* logits; int64_t ld; int n_vocab;
  int G, beam_size, max_candidates;
  const ccx_decode_rules* rules;
  ccx_dec_seq_state* state;
  int sample_len;
  int* hist; int* cur_tok; int* pos; int* n_done;
  const void* tok_emb; const void* pos_emb; void* x; int D;
  uint16_t* ind; int ind_ld;
  int* fin_tok; float* fin_score; int* fin_n; int* fin_count;
  int* cand_id; float* cand_lp; int* tok_out; int* parent_out;
  int64_t logits_elems, tok_emb_elems, pos_emb_elems, x_elems;
  const ccx_decode_options* opts;                             /* NULL: the rules alone (appended) */
} ccx_dec_beam_desc;
int ccx_dec_beam_step(ccx_ctx* ctx, const ccx_dec_beam_desc* desc, void* stream);

/* The history rules on their own (csrc/dec_history.hip: dec_history_kernel, one block per row; the rule: ccx_decode_history_options
 * above): edits the device logit rows in place for the rows in the sampling phase (done == 0 and pos >= prompt_len - 1) from their
 * histories hist[row][0 : n_gen].  Checked on the host before the launch, CCX_ERR_ARG (1) naming "ccx_dec_history_step" and the
 * field: 1 <= rows <= 65536, 1 <= n_vocab <= 53248, ld >= n_vocab, logits 4-byte aligned with logits_elems >= (rows - 1) * ld +
 * n_vocab, 1 <= sample_len <= 2048, 0 <= text_end <= n_vocab, repetition_penalty finite and > 0, no_repeat_ngram_size >= 0, every
 * n_gen in [0, sample_len] and done in {0, 1}, history ids of live rows in [0, n_vocab).  Owns and frees its scratch; synchronises
 * the stream. */
typedef struct ccx_dec_history_desc {
  void* logits; int64_t logits_elems;         /* device f32 [rows][ld], in and out */
  int64_t ld; int n_vocab; int rows;
  const ccx_dec_seq_state* state;             /* HOST [rows] */
  const int* hist; int sample_len;            /* HOST [rows][sample_len] */
  int text_end;                               /* rules.eot: ids >= it are never edited */
  float repetition_penalty; int no_repeat_ngram_size;
} ccx_dec_history_desc;
int ccx_dec_history_step(ccx_ctx* ctx, const ccx_dec_history_desc* desc, void* stream);

/* The sequence bias on its own (csrc/dec_bias.hip: dec_bias_kernel, one block per row; the rule: ccx_decode_bias_options above):
 * edits the device logit rows in place for the rows in the sampling phase (done == 0 and pos >= prompt_len - 1) from their histories
 * hist[row][0 : n_gen] under `table` (HOST arrays; an empty table edits nothing).  Checked on the host before the launch,
 * CCX_ERR_ARG (1) naming "ccx_dec_bias_step" and the field: everything ccx_whisper_set_bias_options checks (with text_end in the
 * place of eot), and 1 <= rows <= 65536, 1 <= n_vocab <= 53248, ld >= n_vocab, logits 4-byte aligned with logits_elems >=
 * (rows - 1) * ld + n_vocab, 1 <= sample_len <= 2048, 0 <= text_end <= n_vocab, every n_gen in [0, sample_len] and done in {0, 1},
 * history ids of live rows in [0, n_vocab).  Owns and frees its scratch; synchronises the stream. */
typedef struct ccx_dec_bias_desc {
  void* logits; int64_t logits_elems;         /* device f32 [rows][ld], in and out */
  int64_t ld; int n_vocab; int rows;
  const ccx_dec_seq_state* state;             /* HOST [rows] */
  const int* hist; int sample_len;            /* HOST [rows][sample_len] */
  int text_end;                               /* rules.eot: ids >= it are never a target */
  ccx_decode_bias_options table;
} ccx_dec_bias_desc;
int ccx_dec_bias_step(ccx_ctx* ctx, const ccx_dec_bias_desc* desc, void* stream);

/* Softmax of logit rows over an id range (csrc/dec_probs.hip: dec_token_probs_kernel, one block per row).  Over the ids [lo, hi) only --
 * everything else, the columns [n_vocab, ld) included, counts as -inf and is never looked at: argmax[row] (lowest id on equal values,
 * as the select kernel and torch.argmax on the CPU), pick_prob[row] = softmax probability of the id `pick`, and, if probs != NULL,
 * probs[row][hi - lo].  fp32, max-subtracted; -inf inside the range contributes 0.  n_vocab need not be a multiple of 4.
 * The model uses it for the no-speech probability at the SOT position (lo = 0, hi = n_vocab, pick = <|nospeech|>; decoding.py
 * `logits[:, self.sot_index].float().softmax(dim=-1)[:, tokenizer.no_speech]`) and for language detection (the contiguous language
 * tokens; decoding.py::detect_language).  Checked on the host before the launch, CCX_ERR_ARG (1) naming "ccx_dec_token_probs" and the
 * field: 1 <= rows <= 65536, 1 <= n_vocab <= 53248, ld >= n_vocab and a multiple of 4, 0 <= lo < hi <= n_vocab, lo <= pick < hi, logits
 * 16-byte aligned with logits_elems >= (rows - 1) * ld + hi rounded up to 4, probs (if given) 4-byte aligned with probs_elems >=
 * rows * (hi - lo).  Owns and frees its scratch; synchronises the stream. */
typedef struct ccx_dec_token_probs_desc {
  const void* logits; int64_t logits_elems;   /* device f32 [rows][ld] */
  int64_t ld; int n_vocab; int rows;
  int lo, hi, pick;
  int* argmax; float* pick_prob;              /* HOST [rows], out */
  void* probs; int64_t probs_elems;           /* optional device f32 [rows][hi - lo], out */
} ccx_dec_token_probs_desc;
int ccx_dec_token_probs(ccx_ctx* ctx, const ccx_dec_token_probs_desc* desc, void* stream);

/* Probability of ONE picked id per logit row (csrc/dec_probs.hip: dec_pick_probs_kernel, one block per row, the row pass of
 * dec_token_probs_kernel): out[row * out_stride] = exp(x[pick] - max) / sum_{j < hi} exp(x[j] - max) with pick = picks[row *
 * pick_stride], over the ids [0, hi) only -- the columns [hi, ld) are never looked at.  fp32, max-subtracted; -inf inside the range
 * contributes 0.  A row whose pick is -1 is skipped: nothing is loaded and nothing is written for it.  hi need not be a multiple of 4.
 * The model uses it for the token probabilities behind a word's `probability` (ccx_whisper_align_probs; openai-whisper
 * timing.py::find_alignment, `logits[len(sot_sequence):, :eot].softmax(dim=-1)[np.arange(len(text_tokens)), text_tokens]`); the
 * strides let it walk column t of [B][T] tables.  Checked on the host before the launch, CCX_ERR_ARG (1) naming "ccx_dec_pick_probs"
 * and the field: 1 <= rows <= 65536, 1 <= hi <= 53248, ld >= hi and a multiple of 4, logits 16-byte aligned with logits_elems >=
 * (rows - 1) * ld + hi rounded up to 4, pick_stride >= 1, out_stride >= 1, picks_elems >= (rows - 1) * pick_stride + 1, out_elems >=
 * (rows - 1) * out_stride + 1.  The picks are copied to the host once before the launch and every value outside {-1} and [0, hi) is
 * refused (a test entry: the model path builds its picks on the host and does not go through here).  Synchronises the stream. */
typedef struct ccx_dec_pick_probs_desc {
  const void* logits; int64_t logits_elems;  /* device f32 [rows][ld] */
  int64_t ld; int rows; int hi;
  const void* picks; int64_t picks_elems; int64_t pick_stride;   /* device int32 */
  void* out; int64_t out_elems; int64_t out_stride;              /* device f32 */
} ccx_dec_pick_probs_desc;
int ccx_dec_pick_probs(ccx_ctx* ctx, const ccx_dec_pick_probs_desc* desc, void* stream);

/* ---- word alignment (csrc/align.hip): what transcribe(word_timestamps=True) of the reference asks for (back/api.py:1435, 1477) --
 * openai-whisper's timing.py::find_alignment [UPSTREAM-RECALL]: cross-attention probabilities of the alignment heads over the first
 * num_frames // 2 encoder positions, standardised over the tokens, median-filtered over the frames, averaged over the heads, and a
 * dynamic-time-warping pass over the negated result.  OPT-IN: nothing of it runs unless ccx_whisper_align / ccx_align_op is called.
 *
 * ccx_align_op runs ONE of the three production launchers on caller-supplied device buffers (kernel parity tests; back/api.py:1435,
 * 1477).  Everything the kernels assume is checked on the host before anything is launched; a violation returns CCX_ERR_ARG (1) with
 * a message naming "ccx_align_op" and the field.  Scratch (the DTW trace, the uploaded tables) is freed on every path; the stream is
 * synchronised. */
#define CCX_ALIGN_SCORES 0   /* align_scores_kernel: P[s][head0 + i][t][:] = softmax_j(q[s][heads[i]] . k[s][heads[i]][j] / 8), j < n_keys[s]; 0 behind */
#define CCX_ALIGN_MATRIX 1   /* align_matrix_kernel: A[s][t][j] = mean_h median7_j((P - mean_t) / std_t), t < n_rows[s], j < n_keys[s] */
#define CCX_ALIGN_DTW 2      /* align_dtw_kernel: DTW over -A[s][r0 : n_rows[s]][: n_keys[s]], path and jump frames */

typedef struct ccx_align_desc {
  /* op 0: q f32 [n_seq][H][64], k bf16 [n_seq][H][Spad][64] (the layout of the model's cross-attention keys); sequence s is row s */
  const void* q; const void* k;
  int64_t q_elems, k_elems;
  int n_seq, H, Spad;
  const int* heads; int n_heads; int head0;   /* op 0: HOST [n_heads] heads of this launch, each in [0, H); written as heads head0 .. of P */
  int t;                                      /* op 0: token row of P written, in [0, T) */
  /* all ops: P f32 [n_seq][Hsel][T][Mmax] (op 0 out, op 1 in), A f32 [n_seq][T][Mmax] (op 1 out, op 2 in); Hsel <= 96, T <= 448,
   * Mmax <= 1500.  n_keys HOST [n_seq]: keys / frames of each sequence, 1 .. Mmax (op 0: also <= Spad; keys behind are never read) */
  int Hsel, T, Mmax;
  const int* n_keys;
  const int* n_rows;                          /* ops 1, 2: HOST [n_seq].  op 1: token rows, 2 .. T.  op 2: r1 (end of the DTW's rows) */
  int r0;                                     /* op 2: first row of the DTW, 0 <= r0 < r1 <= T */
  void* P; void* A;
  int64_t P_elems, A_elems;
  /* op 2 outputs (device int32): text_idx / time_idx [n_seq][T + Mmax] (the first path_len entries), path_len [n_seq],
   * jump_frame [n_seq][T]: time index of the first path cell of text index i < r1 - r0, -1 behind */
  void* text_idx; void* time_idx; void* path_len; void* jump_frame;
  int64_t text_idx_elems, time_idx_elems, path_len_elems, jump_frame_elems;
} ccx_align_desc;

int ccx_align_op(ccx_ctx* ctx, int op, const ccx_align_desc* desc, void* stream);

/* Word alignment of the B windows currently encoded in the instance (back/api.py:1435, 1477): valid after ccx_whisper_encode and
 * after a decode of the same windows.  A teacher-forced pass over tokens[b][: lens[b]] (host [B][max_len], built as
 * ccx_whisper_decoder_logits builds its pass) on the per-layer K / V form with the query projection as a launch of its own; at every
 * layer that holds a selected head, right after that projection, align_scores_kernel writes the step's row of P.  Then the matrix and
 * DTW kernels with r0 = row0, r1 = lens[b] - 1.
 *   n_frames   host [B]: mel frames of each window, 2 .. 3000 (n_frames // 2 keys enter the softmax)
 *   heads      host [n_heads][2] (layer, head) pairs, n_heads <= 96; P's head axis follows this order
 *   probs_out_dev   optional f32 [B][n_heads][max_len][n_audio_ctx]: P (rows t >= lens[b] come from padding tokens, columns behind
 *                   n_frames // 2 are 0); matrix_out_dev optional f32 [B][max_len][n_audio_ctx]: A (0 outside the valid block)
 *   jump_frame_out  host [B][max_len]: entry i < lens[b] - 1 - row0 = encoder position at which text row row0 + i starts, -1 behind
 * Needs B <= the sequences the K / V caches hold (80 on an instance with the encoder-output cross attention) and lens[b] >= row0 + 2.
 * The workspaces (P, A, the DTW trace) are allocated on the first call, sized from max_batch: an instance that never aligns
 * allocates nothing for it.  P is the large one: min(max_batch, K / V sequences) x n_heads x max(n_text_ctx / 2 + 4, max_len) x
 * n_audio_ctx x 4 bytes, 0.79 GB for small.en's 72 default heads at max_batch 8 and 7.9 GB at 80 sequences; a later call that
 * selects more heads or longer rows frees it and allocates the larger one.  Synchronises the stream. */
int ccx_whisper_align(ccx_whisper* w, const int32_t* tokens, const int32_t* lens, int max_len, int B, const int32_t* n_frames,
                      const int32_t* heads, int n_heads, int row0, float* probs_out_dev, float* matrix_out_dev,
                      int32_t* jump_frame_out, void* stream);
/* ccx_whisper_align that also returns the probability of every text token -- what upstream's find_alignment turns into a word's
 * `probability` (timing.py::find_alignment, `token_probs = logits[len(tokenizer.sot_sequence):, :tokenizer.eot].softmax(dim=-1)`,
 * `text_token_probs = token_probs[np.arange(len(text_tokens)), text_tokens]`).  The pass already writes every step's logits; with
 * token_prob_out != NULL one dec_pick_probs_kernel launch per step reads them: row t of sequence b (row0 <= t <= lens[b] - 3; row
 * row0 holds <|notimestamps|> and predicts the first text token, the last text token's row predicts eot and is not used) gives the
 * softmax probability over the ids [0, prob_hi) of tokens[b][t + 1].  Needs 1 <= prob_hi <= n_vocab (upstream: eot) and every such
 * token below prob_hi.  The pick table and the [B][max_len] output live in the alignment workspace (uploaded / cleared once per call,
 * nothing per step).
 *   token_prob_out  host [B][max_len]: entry i < lens[b] - row0 - 2 = probability of text token i, -1 behind
 * P, A and the jump frames are the bits of a call without probabilities.  With token_prob_out == NULL this IS ccx_whisper_align:
 * nothing more is allocated or launched and prob_hi is ignored. */
int ccx_whisper_align_probs(ccx_whisper* w, const int32_t* tokens, const int32_t* lens, int max_len, int B, const int32_t* n_frames,
                            const int32_t* heads, int n_heads, int row0, float* probs_out_dev, float* matrix_out_dev,
                            int32_t* jump_frame_out, int prob_hi, float* token_prob_out, void* stream);

/* Which cross-attention formulation the last ccx_whisper_decode (or ccx_whisper_detect_language) of this instance ran (measurement / test records; the reference has one
 * formulation, MultiHeadAttention.forward(x, xa) behind back/api.py:1286-1292): 0 = "kv16" (per-layer K / V caches, split-KV kernels,
 * <= 16 sequences), 1 = "kv_stream" (per-layer K / V caches, dec_cross_stream_kernel, 17 - 80 sequences), 2 = "xa_stream" (one pass over
 * the encoder output per layer, csrc/cross_x.hip, more than 80 sequences); -1 before the first decode. */
int ccx_whisper_last_cross_path(ccx_whisper* w);

/* ---- multilingual checkpoints (tiny / base / small / medium: n_vocab 51865; the ids of the 51866-token family work too) ----------
 * Any n_vocab <= 53248 is accepted.  Inside the model the select kernel runs on n_vocab rounded up to 4 with the ids behind n_vocab
 * always suppressed; for a multiple of 4 nothing changes.
 *
 * ccx_whisper_set_sot_tail: n_tail = tokens of the SOT sequence BEHIND <|startoftranscript|> (0 for the English-only models,
 * 2 for [sot, <|lang|>, <|transcribe|> or <|translate|>]; decoding.py `self.sot_index = self.initial_tokens.index(tokenizer.sot)`).
 * 3 with <|notimestamps|> behind them: ccx_decode_options.without_timestamps).
 * Default 0, allowed 0 .. 3 on a multilingual vocabulary (n_vocab >= 51865), 0 .. 2 otherwise.  With n_tail > 0, or with n_vocab not a multiple of 4, the no_speech_prob of ccx_whisper_decode is the
 * softmax probability of rules.no_speech over the ids [0, n_vocab) of the logits at prompt position prompt_len - 1 - n_tail (one more
 * gathered row per sequence in the prefill, one logits GEMM over those rows and dec_token_probs_kernel, all before the captured
 * steps); every prompt must then be longer than n_tail tokens and is prefilled -- CCX_PREFILL=0 (a debugging switch) is refused with
 * CCX_ERR_ARG.  With n_tail == 0 and n_vocab a multiple of 4 a decode issues exactly the launches it issued before. */
int ccx_whisper_set_sot_tail(ccx_whisper* w, int n_tail);
/* DecodingOptions.prefix [UPSTREAM-RECALL: decoding.py::_get_initial_tokens]: the last n_prefix tokens of every prompt stand BEHIND the
 * SOT sequence -- part of the prompt, so the first-step rules apply to the first token sampled after them -- and the no-speech
 * probability is read at prompt position prompt_len - 1 - n_tail - n_prefix, as above (n_prefix > 0 takes the same path as n_tail > 0).
 * Sticky; default 0, allowed 0 .. n_text_ctx / 2; every prompt must be longer than n_tail + n_prefix tokens. */
int ccx_whisper_set_prefix_len(ccx_whisper* w, int n_prefix);
/* whisper.decoding.detect_language (what transcribe(language=None), upstream's default and the reference's call at
 * back/api.py:1286-1292, runs on the first window) for the B windows currently encoded: one decoder pass over the single token
 * rules.sot at position 0 -- the step kernels and the cross-attention path (ccx_whisper_last_cross_path, which this call sets) of a
 * decode of B rows, run as one lane whatever B is (large decodes split into lanes; a row's numbers do not depend on the split) and on
 * the instance's own stream when `stream` is NULL, as ccx_whisper_decode does -- then the logits GEMM and
 * dec_token_probs_kernel over the ids [lang_begin, lang_begin + n_lang) (n_lang <= 128; upstream's language tokens are contiguous).
 * lang_token_out host [B]: the most probable language token; probs_out host [B][n_lang] or NULL: the distribution over the range.
 * Leaves the encoder output as it found it: a ccx_whisper_decode of the same windows afterwards returns what it returns without
 * this call.  Valid for every B a decode accepts.  Synchronises the stream. */
int ccx_whisper_detect_language(ccx_whisper* w, int B, int lang_begin, int n_lang, int32_t* lang_token_out, float* probs_out,
                                void* stream);

/* Batch-driver helper with no counterpart in the reference (it decodes one window at a time, back/api.py:1286): picks, once, the
 * internal streams on which the lanes of a large decode batch will run beside `stream` (HIP maps streams onto a few hardware
 * queues; the choice is made by a short timing probe, which must not be disturbed by other work on the GPU).  Call it on an
 * otherwise idle device before decodes are overlapped with other streams; ccx_whisper_decode does it lazily otherwise. */
int ccx_whisper_prepare_lanes(ccx_whisper* w, void* stream);
/* Measurement helper (no counterpart in the reference): while `path` is non-NULL every hipGraph-captured decode step carries
 * one-thread stamp kernels (100 MHz s_memrealtime) around the cross attention of every layer (level 1) or after every kernel of
 * the chain (level 2), per decode lane; each ccx_whisper_decode appends its trace to `path` ("decode B <n> lanes <l>" + one line
 * per lane; tools/decode_stamps.py, bench.py `roofline.frac_in_situ`).  NULL switches it off.  The stamp level is part
 * of the step plan: traced and untraced step graphs live side by side.  Equivalent to creating the model with CCX_DEC_STAMPS=<path> in the environment. */
int ccx_whisper_trace_lanes(ccx_whisper* w, const char* path, int level);

/* ---- RE-SepFormer separator (replaces self.separator, reference back/api.py:713-717; call at
 *      back/api.py:1077 `separated = self.separator.separate_batch(subsegment)`) -------------------- */

typedef struct ccx_sepformer ccx_sepformer;
typedef struct {
  int n_filters, kernel, stride, d_model, n_head, d_ffn, n_layers, n_blocks, segment, n_spk;
} ccx_sepformer_dims;

/* max_tokens: capacity in encoder frames summed over the utterances of one call (each padded to
 * whole `segment`-frame chunks); max_utts: utterances per call.  The geometry is RE-SepFormer's (128 filters, kernel 16, stride 8,
 * d_model 128, 8 heads) with n_spk in [1, 4] sources: `masknet.model.output_fc.1` then has 128 n_spk rows, row c n_spk + s the mask
 * of channel c for source s. */
int ccx_sepformer_create(ccx_ctx* ctx, const ccx_sepformer_dims* dims, int max_tokens, int max_utts,
                         ccx_sepformer** out);
void ccx_sepformer_destroy(ccx_sepformer* s);
/* Tensors by SpeechBrain checkpoint key, prefixed with the module name of the reference's overlay
 * files (back/api.py:729): "encoder.conv1d.weight", "decoder.weight", "masknet.model....". f32. */
int ccx_sepformer_set_tensor(ccx_sepformer* s, const char* name, const float* data, int64_t numel);
int ccx_sepformer_finalize(ccx_sepformer* s);
/* separate_batch for B independent utterances: mix_dev [B, stride] f32, n_samples host [B] ->
 * out_dev [B, stride, n_spk] f32, the sources interleaved per sample (rows past n_samples[b] are zero for every source).  n_spk
 * is the handle's (ccx_sepformer_dims, 1 to 4; 2 for the model the reference loads): the mask head is one GEMM of 128 n_spk
 * columns, the decoder one instantiation per n_spk. */
int ccx_sepformer_separate(ccx_sepformer* s, const float* mix_dev, int64_t stride, const int* n_samples, int B,
                           float* out_dev, void* stream);

/* ---- the SepFormer layer kernels on their own (csrc/sepformer.hip through the launchers of csrc/sepformer.h; for kernel parity
 *      tests, the product path does not call this) -------------------------------------------------------------------------
 * One descriptor, one op code.  Device pointers come with the element count (of the buffer's own type) behind them; sequence and
 * utterance tables are HOST arrays, checked and uploaded into scratch that is freed on every path.  Everything the kernels assume is
 * checked on the host before anything is launched; a violation returns CCX_ERR_ARG (1) with a message naming "ccx_sep_op" and the
 * field.  Synchronises the stream. */
#define CCX_SEP_ATTN_BLOCK 0   /* sep_attn_block_kernel: h += out_proj(attention(LN(h) Wqkv^T + bqkv)) + bo per sequence, len <= 160 */
#define CCX_SEP_ATTENTION 1    /* sep_attention_kernel: qkv -> att per sequence and head, any len */
#define CCX_SEP_FFN 2          /* sep_ffn_kernel: h[0 .. n_tok) += W2 relu(W1 LN(h) + b1) + b2 */
#define CCX_SEP_FINAL_NORM 3   /* sep_final_norm_kernel: y = gLN(LN(h)) + xin per sequence */
#define CCX_SEP_DECODER 4      /* sep_decoder_kernel<n_spk>: out[u][t][spk] from feats * relu(fc), 16 taps, stride 8 */

typedef struct ccx_sep_desc {
  /* token buffers, `rows` rows each: h f32 [rows][128] (ops 0, 2: in and out; op 3: in), xin / y f32 [rows][128] (op 3: skip input /
   * output), qkv bf16 [rows][384] and att bf16 [rows][128] (op 1), feats f32 [rows][128] and fc f32 [rows][128 n_spk] (op 4:
   * column c n_spk + s is the mask logit of channel c for source s) */
  void* h; const void* xin; void* y; const void* qkv; void* att; const void* feats; const void* fc;
  int64_t h_elems, xin_elems, y_elems, qkv_elems, att_elems, feats_elems, fc_elems;
  int rows;
  /* ops 0, 1, 3: HOST tables of n_seq sequences (start row, len >= 1), each inside [0, rows); pairwise disjoint for op 0 */
  const int* seq_start; const int* seq_len; int n_seq;
  /* op 2: tokens [0, n_tok) of h, n_tok >= 1; d_ffn a multiple of 64 in [64, 1024] */
  int n_tok, d_ffn;
  /* parameters: ln_g / ln_b f32 [128] (ops 0, 2, 3), gln_g / gln_b f32 [128] (op 3); op 0: wqkv bf16 [384][128], bqkv f32 [384],
   * wo bf16 [128][128], bo f32 [128]; op 2: w1 bf16 [d_ffn][128], b1 f32 [d_ffn], w2 bf16 [128][d_ffn], b2 f32 [128];
   * op 4: wdec f32 [128][16] */
  const void* ln_g; const void* ln_b; const void* gln_g; const void* gln_b;
  const void* wqkv; const void* bqkv; const void* wo; const void* bo;
  const void* w1; const void* b1; const void* w2; const void* b2; const void* wdec;
  int64_t ln_elems, gln_elems, wqkv_elems, bqkv_elems, wo_elems, bo_elems, w1_elems, b1_elems, w2_elems, b2_elems, wdec_elems;
  /* op 4: HOST tables of n_utt utterances: first token row, frames L >= 1, samples 16 <= T <= out_stride; an utterance owns the rows
   * of its frames padded to whole `segment`-row chunks (a full extra chunk when L is a multiple of it), all inside [0, rows).
   * out f32 [n_utt][out_stride][n_spk] */
  const int* utt_tok0; const int* utt_L; const int* utt_T; int n_utt; int segment;
  void* out; int64_t out_stride; int64_t out_elems;
  /* op 4: sources of the mask and of out, 1 to 4; 0 means 2 (a descriptor written before the field existed).  Anything else is
   * CCX_ERR_ARG; fc_elems and out_elems are checked against it */
  int n_spk;
} ccx_sep_desc;

int ccx_sep_op(ccx_ctx* ctx, int op, const ccx_sep_desc* desc, void* stream);

/* ---- dual-path SepFormer separator (SpeechBrain's Dual_Path_Model: sepformer-wsj02mix / -wsj03mix / -wham / -whamr / -libri2mix /
 *      -libri3mix and the one-source enhancement models; csrc/dualpath.hip).  Opt-in: nothing else of the library calls it. -----
 * Restated from recollection [UPSTREAM-RECALL], parity unpinned (tests/dualpath_reference.py is the fp64 statement it is checked
 * against).  The geometry: n_filters == d_model == 256, n_head == 8 (heads of 32), kernel even in [2, 32] with stride == kernel / 2,
 * segment K even in [2, 256] (chunks at 50 % overlap), d_ffn a multiple of 64 in [64, 2048], n_layers and n_blocks in [1, 8], n_spk
 * in [1, 3]; anything else is CCX_ERR_ARG naming the field, before any allocation.  max_tokens counts chunk rows, S K per utterance
 * with S = 2 (L + gap + K / 2) / K chunks, gap = K - (K / 2 + L % K) % K, L = (T - kernel) / stride + 1 frames. */
typedef struct ccx_dualpath ccx_dualpath;
typedef struct {
  int n_filters, kernel, stride, d_model, n_head, d_ffn, n_layers, n_blocks, segment, n_spk;
} ccx_dualpath_dims;

int ccx_dualpath_create(ccx_ctx* ctx, const ccx_dualpath_dims* dims, int max_tokens, int max_utts, ccx_dualpath** out);
void ccx_dualpath_destroy(ccx_dualpath* s);
/* Tensors by SpeechBrain checkpoint key with the module prefix: "encoder.conv1d.weight", "decoder.weight", "masknet.norm.weight",
 * "masknet.conv1d.weight", "masknet.dual_mdl.<b>.{intra,inter}_mdl.mdl.layers.<l>....", "masknet.dual_mdl.<b>.{intra,inter}_norm.*",
 * "masknet.prelu.weight", "masknet.conv2d.*" (row s 256 + c: source s, channel c), "masknet.output.0.*", "masknet.output_gate.0.*",
 * "masknet.end_conv1x1.weight".  f32.  "....pos_enc.pe" buffers of the transformers are accepted and ignored; "masknet.pos_enc.*"
 * (use_global_pos_enc) and "....intra_linear.*" / "....inter_linear.*" (linear_layer_after_inter_intra) are refused by name. */
int ccx_dualpath_set_tensor(ccx_dualpath* s, const char* name, const float* data, int64_t numel);
int ccx_dualpath_finalize(ccx_dualpath* s);
/* mix_dev [B, stride] f32, n_samples host [B] (kernel <= n_samples[b] <= stride) -> out_dev [B, stride, n_spk] f32, the sources
 * interleaved per sample, zero from n_samples[b] on.  Rows are independent utterances. */
int ccx_dualpath_separate(ccx_dualpath* s, const float* mix_dev, int64_t stride, const int* n_samples, int B, float* out_dev,
                          void* stream);

/* ---- the dual-path kernels on their own (for kernel parity tests; the product path does not call this).  One descriptor, one op
 *      code.  Device pointers come with the element count (of the buffer's own type) behind them; tables are HOST arrays, checked
 *      and uploaded into scratch that is freed on every path.  Everything the kernels assume is checked on the host before anything is
 *      launched; a violation returns CCX_ERR_ARG (1) with a message naming "ccx_dualpath_op" and the field.  Synchronises the stream.
 *      `rows` is the row count of token buffers, `frames` of frame buffers; every row holds 256 channels unless stated. */
#define CCX_DP_ATTENTION 0    /* in = qkv bf16 [rows][768] -> out bf16 [rows][256]; seq_first / seq_stride / seq_len [n_seq] */
#define CCX_DP_GROUP_NORM 1   /* in f32 [rows][256], utterance u = rows [utt_row0[u], + utt_rows[u]); w = gamma, w2 = beta f32 [256].
                                 mode 0: out f32 = norm + in2 (skip, f32 [rows][256]; may be `out` itself); mode 1: out bf16, no skip */
#define CCX_DP_SEGMENT 2      /* in f32 [frames][256] -> out f32 [rows][256]: chunks of `segment` at 50 % overlap, padding zeroed */
#define CCX_DP_OVERLAP_ADD 3  /* in f32 [rows][256 n_spk] -> out bf16 [frames n_spk][256], row (frame0 + l) n_spk + s */
#define CCX_DP_PE_ADD 4       /* out f32 = in f32 + w[pos][:], pos = position in the chunk (mode 0) or chunk index (mode 1); w f32 [.][256] */
#define CCX_DP_GATE 5         /* in f32 [rows][512] -> out bf16 [rows][256] = tanh(in[r][c]) sigmoid(in[r][256 + c]) */
#define CCX_DP_ENCODER 6      /* in = mix f32 [n_utt][in_stride], w f32 [256][kernel] -> out f32 [frames][256], ReLU */
#define CCX_DP_DECODER 7      /* in = feats f32 [frames][256], in2 = mask f32 [frames n_spk][256], w = wdec f32 [256][kernel]
                                 -> out f32 [n_utt][out_stride][n_spk] */
#define CCX_DP_PRELU 8        /* in f32 [rows][256], w = slope f32 [1] -> out bf16 [rows][256] */

typedef struct ccx_dualpath_desc {
  const void* in; const void* in2; void* out; const void* w; const void* w2;
  int64_t in_elems, in2_elems, out_elems, w_elems, w2_elems;
  int rows, frames, mode;
  /* op 0: HOST tables of n_seq sequences: first row >= 0, row stride >= 1, length >= 1, the last row inside [0, rows) */
  const int* seq_first; const int* seq_stride; const int* seq_len; int n_seq;
  /* op 1: HOST tables of n_utt row ranges inside [0, rows) */
  const int* utt_row0; const int* utt_rows;
  /* ops 2, 3, 4: HOST tables of n_utt utterances: first token row, first frame row, frames L >= 1, gap and S as the rule above gives
   * them for `segment` (checked), the S segment rows inside [0, rows), the L frames inside [0, frames).  ops 6, 7: utt_frame0, utt_L
   * and samples utt_T; op 6: utt_L == (utt_T - kernel) / (kernel / 2) + 1, utt_T <= in_stride; op 7: 1 <= utt_T <= out_stride */
  const int* utt_tok0; const int* utt_frame0; const int* utt_L; const int* utt_gap; const int* utt_S; const int* utt_T; int n_utt;
  int segment, kernel, n_spk;
  int64_t in_stride, out_stride;
} ccx_dualpath_desc;

int ccx_dualpath_op(ccx_ctx* ctx, int op, const ccx_dualpath_desc* desc, void* stream);

/* ---- pyannote-style speaker networks (replace self.embedding_model = Inference("pyannote/embedding",
 *      window="whole"), reference back/api.py:776-780, called at back/api.py:869; and the segmentation
 *      network inside self.vad_pipeline / self.diarization, reference back/api.py:782-792, called at
 *      back/api.py:1311, 1056, 1124) ------------------------------------------------------------------ */

typedef struct ccx_speaker ccx_speaker;
/* kind 0: XVectorSincNet embedder (512-d).  kind 1: PyanNet segmentation (n_classes per frame; powerset
 * != 0 -> log-softmax, else sigmoid).  max_samples: total samples of all crops of one call. */
int ccx_speaker_create(ccx_ctx* ctx, int kind, int n_classes, int powerset, int max_crops, int64_t max_samples,
                       ccx_speaker** out);
void ccx_speaker_destroy(ccx_speaker* s);
/* Tensors by pyannote checkpoint key (f32): "sincnet.wav_norm1d.weight", "sincnet.conv1d.0.filters"
 * ([80,251] band-pass filters expanded from low_hz_/band_hz_ by the host), "sincnet.conv1d.1.weight", ...,
 * "tdnns.N.0.weight", "tdnns.N.2.running_mean", "embedding.weight" | "lstm.weight_ih_l0_reverse",
 * "linear.0.weight", "classifier.weight". */
int ccx_speaker_set_tensor(ccx_speaker* s, const char* name, const float* data, int64_t numel);
int ccx_speaker_finalize(ccx_speaker* s);
/* n crops stored in wav_dev at sample offsets[i], n_samples[i] long (host arrays) -> out_dev [n, 512] f32.
 * weights_dev (optional, NULL = plain mean/std pooling): per-crop frame weights at any resolution
 * (w_lens[i] values at w_offsets[i]), nearest-interpolated to the pooling frames (pyannote StatsPool). */
int ccx_speaker_embed(ccx_speaker* s, const float* wav_dev, const int64_t* offsets, const int* n_samples, int n,
                      const float* weights_dev, const int64_t* w_offsets, const int* w_lens, float* out_dev, void* stream);
/* per-frame class scores of n crops, concatenated in crop order: out_dev [sum frames, n_classes] f32;
 * frames_out[i] (host) = frames of crop i. */
int ccx_speaker_segment(ccx_speaker* s, const float* wav_dev, const int64_t* offsets, const int* n_samples, int n,
                        float* out_dev, int64_t out_capacity_rows, int* frames_out, void* stream);

/* ---- the SincNet / x-vector / PyanNet kernels on their own (csrc/speaker.hip through the launch functions and weight packers
 *      ccx_speaker_embed and ccx_speaker_segment use; for kernel parity tests, the product path does not call this; no counterpart
 *      in the reference).  Device pointers come with the element count of the buffer's own type; crop tables, the sinc filters and
 *      W_hh are HOST arrays.  Everything the kernels assume is checked on the host before anything is launched; a violation returns
 *      CCX_ERR_ARG (1) with a message naming "ccx_speaker_op" and the field.  Synchronises the stream.
 *      Ragged rows: crop i reads frames of `in` from row in_off[i] and writes frames[i] rows of `out` from row out_off[i]. */
#define CCX_SPEAKER_WAV_STATS 0   /* wav_stats_kernel: wav crops -> out f32 [n][4] = (a, c, mean_hi, mean_lo): the norm is a x + c, the mean mean_hi + mean_lo */
#define CCX_SPEAKER_SINC_POOL 1   /* wav_stats_kernel + sinc_conv_pool_kernel: wav crops -> out f32 [.][80], frames[i] pooled frames */
#define CCX_SPEAKER_INORM 2       /* inorm_partial_kernel + inorm_apply_kernel<pool>: in f32 [.][ld_in] -> out bf16 [.][ld_out] */
#define CCX_SPEAKER_STATS_POOL 3  /* stats_pool_kernel: in bf16 [.][ld_in] -> out bf16 [n][ld_out] (mean at [0, C) || std at [C, 2 C)) */
#define CCX_SPEAKER_LSTM 4        /* lstm_recurrent_kernel: in = gx f32 [.][1024] (fwd | rev gates i|f|g|o) -> out = h bf16 [.][256] */
#define CCX_SPEAKER_ACTIVATION 5  /* seg_activation_kernel: in = logits f32 [rows][ld_in] -> out f32 [rows][C] */

typedef struct ccx_speaker_desc {
  int n;                        /* ops 0-4: crops (sequences), 1..65535 */
  /* ops 0, 1: wav f32 (4-byte aligned); HOST crop_off (samples, >= 0) and crop_len (>= 251) [n]; the waveform norm's weight and bias */
  const void* wav; int64_t wav_elems; const int64_t* crop_off; const int* crop_len; float norm_w, norm_b;
  /* op 1: HOST sinc filters f32 [80][251], packed into MFMA fragments as the loader does */
  const float* filters_host;
  /* ops 1-4: HOST frames [n].  op 1: pooled frames written, 1 .. ((crop_len - 251) / 10 + 1) / 3.  op 2: frames after the pool
   * (pool x frames input rows are read).  op 3: frames pooled over (>= 2 without weights).  op 4: steps of the sequence. */
  const int* frames;
  /* ops 2-5: in, with ld_in elements per row; ops 2-4: HOST in_off [n], the first input row of each crop */
  const void* in; int64_t in_elems; int64_t ld_in; const int* in_off;
  /* all ops: out.  ops 1, 2, 4: HOST out_off [n], the first output row of each crop (op 1: rows are 80 wide; op 4: out_off must
   * equal in_off).  ops 2, 3: ld_out elements per row (op 2: columns [C, ld_out) are written as zeros). */
  void* out; int64_t out_elems; int64_t ld_out; const int* out_off;
  /* op 2: pool 1 or 3 (max over 3 input rows first); C live channels, a multiple of 4, <= ld_in, <= ld_out <= 128; ld_in and ld_out
   * multiples of 4; gamma / beta f32 [C] (device).  ops 3, 5: C columns. */
  int pool, C; const void* gamma; int64_t gamma_elems; const void* beta; int64_t beta_elems;
  /* op 3: weights f32 (device, may be NULL: unbiased std); HOST w_off / w_len [n]: w_len[i] >= 1 weights at w_off[i], nearest-
   * interpolated to the crop's frames */
  const void* weights; int64_t weights_elems; const int64_t* w_off; const int* w_len;
  /* op 4: HOST whh f32 [2][512][128] (fwd | rev, rows i|f|g|o), rounded to bf16 as the loader does */
  const float* whh_host;
  /* op 5: rows; powerset != 0 -> log-softmax over the C columns, else sigmoid */
  int rows, powerset;
} ccx_speaker_desc;

int ccx_speaker_op(ccx_ctx* ctx, int op, const ccx_speaker_desc* desc, void* stream);

/* ---- ECAPA-TDNN speaker embedder (speechbrain/spkrec-ecapa-voxceleb, 192-d): an alternative to the x-vector above for
 *      self.embedding_model (reference back/api.py:776-780), called with the same crops (back/api.py:869-872, 961-1006).
 *      The reference itself does not use it; it is selected with load_models(embedding="ecapa"). ------------------------- */
typedef struct ccx_ecapa ccx_ecapa;
/* max_samples: total samples of all crops of one call (replaces the model construction at back/api.py:776-780) */
int ccx_ecapa_create(ccx_ctx* ctx, int max_crops, int64_t max_samples, ccx_ecapa** out);
void ccx_ecapa_destroy(ccx_ecapa* e);
/* Tensors by speechbrain checkpoint key (f32): "blocks.0.conv.conv.weight", "blocks.1.res2net_block.blocks.0.norm.norm.running_var",
 * "blocks.1.se_block.conv1.conv.weight", "mfa.conv.conv.weight", "asp.tdnn.conv.conv.weight", "asp.conv.conv.weight",
 * "asp_bn.norm.weight", "fc.conv.weight", ... and the two host-computed front-end tables "fbank.window" [400] and "fbank.filters"
 * [80][201] (replaces EncoderClassifier's checkpoint loading; the reference has no counterpart). */
int ccx_ecapa_set_tensor(ccx_ecapa* e, const char* name, const float* data, int64_t numel);
int ccx_ecapa_finalize(ccx_ecapa* e);
/* n crops stored in wav_dev at sample offsets[i], n_samples[i] >= 8000 long (host arrays, the convention of ccx_speaker_embed)
 * -> out_dev [n, 192] f32.  Every crop is its own utterance (replaces the call at back/api.py:869-872). */
int ccx_ecapa_embed(ccx_ecapa* e, const float* wav_dev, const int64_t* offsets, const int* n_samples, int n, float* out_dev,
                    void* stream);

/* ---- the ECAPA-TDNN kernels on their own (csrc/ecapa.hip through the launchers of csrc/ecapa.h; for kernel parity tests, the
 *      product path does not call this; no counterpart in the reference).  Device pointers come with the element count of the buffer's
 *      own type; crop tables and the Res2Net weights are HOST arrays.  Everything the kernels assume is checked on the host before
 *      anything is launched; a violation returns CCX_ERR_ARG (1) with a message naming "ccx_ecapa_op" and the field.  Synchronises
 *      the stream.
 *      Rows: crop i owns rows row_off[i] .. row_off[i] + frames[i] + 8 of every [rows][C] buffer (4 halo rows, frames, 4 halo rows). */
#define CCX_ECAPA_FBANK 0      /* ecapa_fbank_kernel + mean + apply: wav -> feats bf16 [rows][80] with halos */
#define CCX_ECAPA_RES2NET 1    /* ecapa_res2net_kernel: x [rows][ldx] -> y [rows][ldy], 1024 columns, halos written */
#define CCX_ECAPA_SE 2         /* ecapa_se_mean / excite / apply: y = gates * x + resid, gates f32 [n][1024] (optional output) */
#define CCX_ECAPA_ASP_POOL 3   /* ecapa_asp_pool_kernel: hidden [rows][128], x [rows][ldx] -> pooled bf16 [n][2 channels] */

typedef struct ccx_ecapa_desc {
  /* HOST crop tables: n crops, first row and frame count (>= 5) of each; crops pairwise disjoint inside [0, rows) */
  int n; const int* row_off; const int* frames; int rows;
  /* op 0: wav f32, HOST offsets / n_samples (>= 8000 each; frames[i] must be 1 + n_samples[i] / 160), window f32 [400],
   * filters f32 [80][201] (device), feats bf16 [rows][80] */
  const void* wav; int64_t wav_elems; const int64_t* offsets; const int* n_samples;
  const void* window; int64_t window_elems; const void* filters; int64_t filters_elems;
  void* feats; int64_t feats_elems;
  /* ops 1, 2, 3: x bf16 [rows][ldx] in; ops 1, 2: y bf16 [rows][ldy] out (1024 live columns each; ld a multiple of 8) */
  const void* x; int64_t x_elems; int64_t ldx; void* y; int64_t y_elems; int64_t ldy;
  /* op 1: dilation 1..4; HOST conv weights f32 [7][128][128][3] and HOST (bias | scale | shift) f32 [7][3][128] */
  int dilation; const float* w_host; const float* aff_host;
  /* op 2: resid bf16 [rows][ld_resid]; w1 f32 [128][1024], b1 f32 [128], w2 f32 [1024][128], b2 f32 [1024] (device);
   * gates f32 [n][1024] (device, may be NULL) */
  const void* resid; int64_t resid_elems; int64_t ld_resid;
  const void* w1; const void* b1; const void* w2; const void* b2; int64_t w1_elems, b1_elems, w2_elems, b2_elems;
  void* gates; int64_t gates_elems;
  /* op 3: channels (a multiple of 64, <= ldx); hidden bf16 [rows][128]; wa bf16 [channels][128], ba f32 [channels], bn_scale /
   * bn_shift f32 [2 channels] (device); pooled bf16 [n][2 channels] */
  int channels; const void* hidden; int64_t hidden_elems;
  const void* wa; const void* ba; const void* bn_scale; const void* bn_shift; int64_t wa_elems, ba_elems, bn_elems;
  void* pooled; int64_t pooled_elems;
} ccx_ecapa_desc;

int ccx_ecapa_op(ccx_ctx* ctx, int op, const ccx_ecapa_desc* desc, void* stream);

/* ---- WeSpeaker ResNet-34 speaker embedder: the embedding model inside self.diarization =
 *      Pipeline.from_pretrained("pyannote/speaker-diarization-3.1"), reference back/api.py:788-792, called at
 *      back/api.py:1056-1060 and 1124-1128 (one embedding per 10 s chunk and local speaker) ---------------- */
typedef struct ccx_resnet ccx_resnet;
/* max_samples: longest chunk of one call; max_masks: most (chunk, speaker) masks of one call */
int ccx_resnet_create(ccx_ctx* ctx, int max_chunks, int64_t max_samples, int max_masks, ccx_resnet** out);
void ccx_resnet_destroy(ccx_resnet* r);
/* Tensors by checkpoint key (f32): "resnet.conv1.weight", "resnet.bn1.running_mean", "resnet.layer2.0.conv1.weight",
 * "resnet.layer2.0.shortcut.0.weight", "resnet.layer2.0.shortcut.1.weight", ..., "resnet.seg_1.weight". */
int ccx_resnet_set_tensor(ccx_resnet* r, const char* name, const float* data, int64_t numel);
int ccx_resnet_finalize(ccx_resnet* r);
/* wav_dev [n_chunks, stride] f32, every chunk n_samples long.  weights_dev NULL: one embedding per chunk, out_dev
 * [n_chunks, 256] f32.  Else weights_dev [n_masks, n_w] f32 frame weights (any resolution, nearest-interpolated to
 * the pooling frames) and mask_chunk [n_masks] (host: the chunk each mask pools over): out_dev [n_masks, 256].
 * The convolutional trunk runs once per chunk. */
int ccx_resnet_embed(ccx_resnet* r, const float* wav_dev, int64_t stride, int n_samples, int n_chunks, const float* weights_dev,
                     int n_w, const int* mask_chunk, int n_masks, float* out_dev, void* stream);

/* ---- the ResNet-34 kernels on their own (csrc/resnet.hip through the launch functions ccx_resnet_embed uses; for kernel parity
 *      tests, the product path does not call this; no counterpart in the reference).  Device pointers come with the element count of
 *      the buffer's own type; convolution weights and mask_chunk are HOST arrays.  Everything the kernels assume is checked on the host
 *      before anything is launched; a violation returns CCX_ERR_ARG (1) with a message naming "ccx_resnet_op" and the field.
 *      Synchronises the stream.
 *      Padded layout: bf16 [chunk][H + 2][W + 2][C], a one-pixel halo around every image. */
#define CCX_RESNET_FBANK 0      /* fbank_kernel + fbank_mean_kernel: wav -> feats_t f32 [chunk][80][T], fmean f32 [chunk][80] */
#define CCX_RESNET_CONV1 1      /* conv1_kernel: feats_t, fmean -> out, padded [chunk][82][T + 2][32] (interior only) */
#define CCX_RESNET_CONV 2       /* one folded convolution of the trunk, dispatched as the product does (direct kernel or GEMM) */
#define CCX_RESNET_HALO_ZERO 3  /* halo_zero_kernel: halo cells of chunks [c0, c0 + n) of three padded buffers */
#define CCX_RESNET_TSTP 4       /* tstp_kernel: act, padded [chunk][12][W4 + 2][256] -> pooled f32 [n_masks][5120] */
#define CCX_RESNET_LINEAR 5     /* embed_linear_kernel: pooled -> emb f32 [n_masks][256] */
#define CCX_RESNET_EPI_PLAIN 0     /* out = conv + shift */
#define CCX_RESNET_EPI_RELU 1      /* out = relu(conv + shift) */
#define CCX_RESNET_EPI_ADD_RELU 2  /* out = relu(conv + shift + resid) */

typedef struct ccx_resnet_desc {
  int n_chunks;                 /* ops 0, 1, 2, 4 */
  /* op 0: wav f32 [n_chunks][stride], the first n_samples (>= 400) of every row are read; T = 1 + (n_samples - 400) / 160.
   * ops 0, 1: feats_t f32 [n_chunks][80][T], fmean f32 [n_chunks][80] (op 0 writes them, op 1 reads them) */
  const void* wav; int64_t wav_elems; int64_t stride; int n_samples;
  void* feats_t; int64_t feats_t_elems; void* fmean; int64_t fmean_elems;
  /* op 1: T frames; c1w f32 [32][9] and c1b f32 [32] (device, BatchNorm folded); writes out */
  int T; const void* c1w; int64_t c1w_elems; const void* c1b; int64_t c1b_elems;
  /* op 2: (cin, cout, k, conv_stride) one of the network's: k 3 stride 1 with cin == cout in {32, 64, 128, 256}, or k 3 / k 1
   * stride 2 with (cin, cout) in {(32, 64), (64, 128), (128, 256)}.  H (even) x W (>= 2) is the INPUT image; the output image is
   * H x W (stride 1) or H / 2 x ((W - 1) / 2 + 1) (stride 2).  epi: CCX_RESNET_EPI_*.  HOST w_host f32 [cout][cin][k][k] (torch
   * layout), HOST scale_host / shift_host f32 [cout] (the folded BatchNorm).  in / out / resid in the padded layouts of their
   * images; resid (output layout) with ADD_RELU only.  in_elems must cover the read slack of the strided view behind the layout:
   * two padded rows and one K tile (align(k cin, 64) elements).  Only interior cells of out are written. */
  int cin, cout, k, conv_stride, H, W, epi;
  const float* w_host; const float* scale_host; const float* shift_host;
  const void* in; int64_t in_elems; void* out; int64_t out_elems; const void* resid; int64_t resid_elems;
  /* op 3: three buffers [>= c0 + n][H + 2][Wp][C] of halo0_elems elements each, C in {32, 64, 128, 256} (H as above, any >= 1) */
  void* halo0; void* halo1; void* halo2; int64_t halo0_elems; int c0, n, Wp, C;
  /* op 4: act bf16; weights f32 [n_masks][n_w] (device, may be NULL: unbiased std); HOST mask_chunk [n_masks] (the chunk a mask
   * pools over; required with weights; without it n_masks must equal n_chunks).  ops 4, 5: pooled f32 [n_masks][5120] */
  const void* act; int64_t act_elems; int W4;
  const void* weights; int64_t weights_elems; int n_w; const int* mask_chunk; int n_masks;
  void* pooled; int64_t pooled_elems;
  /* op 5: lin_w f32 [256][5120], lin_b f32 [256] (device) -> emb f32 [n_masks][256] */
  const void* lin_w; int64_t lin_w_elems; const void* lin_b; int64_t lin_b_elems; void* emb; int64_t emb_elems;
} ccx_resnet_desc;

int ccx_resnet_op(ccx_ctx* ctx, int op, const ccx_resnet_desc* desc, void* stream);

/* ---- spectral-gate denoiser (replaces nr.reduce_noise(y=, sr=, stationary=True, prop_decrease=),
 *      reference back/api.py:349 and 832-833; the package's other mode and options: *_ex below) ------- */
typedef struct ccx_specgate ccx_specgate;
int ccx_specgate_create(ccx_ctx* ctx, int64_t max_samples, int max_clips, int sample_rate, ccx_specgate** out);
void ccx_specgate_destroy(ccx_specgate* g);
/* y_dev [B, stride] f32, n_samples host [B] -> out_dev [B, stride] f32 (samples past n_samples[b] are zero) */
int ccx_specgate_reduce(ccx_specgate* g, const float* y_dev, int64_t stride, const int* n_samples, int B,
                        float prop_decrease, float* out_dev, void* stream);
/* noisereduce's `clip_noise_stationary` (default on): the noise statistics of ccx_specgate_reduce_long come from the first 600000
 * samples of the signal only (y_noise = y clipped to chunk_size); 0 = from the whole signal.  Parity unpinned (no fixture, the
 * package is not importable): [UPSTREAM-RECALL] says the clip is applied when the signal stands in for the noise clip as well. */
int ccx_specgate_set_clip_noise(ccx_specgate* g, int on);
/* One signal of ANY length (device pointers): noisereduce's chunked path for inputs beyond its chunk_size of 600000 samples --
 * threshold from the noise clip (see above), then each 600000-sample chunk gated with 30000 samples of real context on either side
 * (the reference passes whole files to nr.reduce_noise, back/api.py:832-833).  Capacity: n / 256 + 1 <= frame rows of the
 * workspace = (max_samples + 60000) / 256 + 2 per clip x max_clips.  y_dev and out_dev must not overlap. */
int ccx_specgate_reduce_long(ccx_specgate* g, const float* y_dev, int64_t n, float prop_decrease, float* out_dev, void* stream);

/* ---- the rest of nr.reduce_noise: non-stationary mode, a separate noise clip, the tunables ---------------------------------------
 * ccx_specgate_reduce / _reduce_long above are ccx_specgate_reduce_ex / _reduce_long_ex with ccx_specgate_opts_default and the
 * caller's prop_decrease: same kernels, same arguments, same bits.
 *
 * stationary = 1 (noisereduce's SpectralGateStationary): threshold = mean + n_std_thresh * std per bin of the dB spectrogram of the
 *   noise clip -- the signal itself (noise_rows = 0), ONE clip shared by all B rows (noise_rows = 1, noise_stride unused) or one per
 *   row (noise_rows = B, clip b at noise_dev + b * noise_stride).  The noise pass is unpadded and floors at 80 dB under the noise
 *   clip's own per-bin maximum.  n_noise is a HOST array of noise_rows lengths, each in [1, max_samples]; in reduce_long_ex the one
 *   clip may be as long as the workspace's frame rows hold and is cut to its first 600000 samples while clip_noise is on.
 * stationary = 0 (SpectralGateNonStationary, the package's default mode; [UPSTREAM-RECALL], PARITY UNPINNED like the stationary mode:
 *   the package is not importable here and no fixture exists; CPU restatement: tests/nonstationary_gate_reference.py).  Per padded
 *   chunk, with the chunking, padding and STFT of the stationary path:
 *     A = |X|;  t = time_constant_s * 16000 / 256;  b = (sqrt(1 + 4 t^2) - 1) / (2 t^2)
 *     S = filtfilt([b], [1, b - 1], A, axis = time, padtype = None)
 *     M = 1 / (1 + exp(-((A - S) / S - thresh_n_mult) * sigmoid_slope)), smoothed with the same 33 x 7 triangle,
 *     then M * prop_decrease + (1 - prop_decrease) -- AFTER smoothing (the stationary mode scales before) -- and out = istft(X * M).
 *   A noise clip is validated and ignored, as upstream ignores it.  DEVIATION: a bin whose S is 0 (an all-zero row; upstream divides
 *   0 by 0 and returns NaN) takes mask 0, so an all-zero signal returns exact zeros.
 * Every field is checked on the host before anything is launched; a violation returns CCX_ERR_ARG (1) with a message naming the
 * field: prop_decrease / n_std_thresh / thresh_n_mult / sigmoid_slope finite, time_constant_s > 0, noise_rows in {0, 1, B},
 * n_noise[i] within capacity and (noise_rows = B) within noise_stride. */
typedef struct ccx_specgate_opts {
  int stationary;
  float prop_decrease;      /* 1.0 */
  float n_std_thresh;       /* n_std_thresh_stationary, 1.5 */
  float time_constant_s;    /* 2.0 */
  float thresh_n_mult;      /* thresh_n_mult_nonstationary, 2.0 */
  float sigmoid_slope;      /* sigmoid_slope_nonstationary, 10.0 */
  const float* noise_dev;   /* device; NULL with noise_rows = 0 */
  int64_t noise_stride;
  const int* n_noise;       /* host [noise_rows] */
  int noise_rows;
} ccx_specgate_opts;
/* stationary = 1, the defaults above, no noise clip */
void ccx_specgate_opts_default(ccx_specgate_opts* opts);
int ccx_specgate_reduce_ex(ccx_specgate* g, const ccx_specgate_opts* opts, const float* y_dev, int64_t stride, const int* n_samples,
                           int B, float* out_dev, void* stream);
int ccx_specgate_reduce_long_ex(ccx_specgate* g, const ccx_specgate_opts* opts, const float* y_dev, int64_t n, float* out_dev,
                                void* stream);
/* Kernel parity tests: exactly the product's time-smoothing launches (csrc/spectral_gate.hip: forward-backward first-order
 * recursion over 64-frame segments, three launches) on a caller's matrices, then a stream synchronise.  a_dev / s_dev: device
 * [B][clip_stride_rows][520] f32 (513 bins used), n_frames host [B], each in [1, min(2580, clip_stride_rows)]; B <= max_clips;
 * b in (0, 1].  Rows at and beyond n_frames[b] of s_dev are not written.  s_dev must not alias a_dev. */
int ccx_specgate_time_smooth(ccx_specgate* g, const float* a_dev, float* s_dev, const int* n_frames, int B, int64_t clip_stride_rows,
                             float b, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CCX_H */

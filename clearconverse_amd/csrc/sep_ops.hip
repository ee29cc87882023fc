// sep_ops.hip -- the SepFormer layer kernels as stand-alone operators of the C ABI (include/ccx.h: ccx_sep_op).  For kernel parity
// tests: the entry point checks on the host everything the kernels assume, uploads the sequence / utterance tables into scratch of
// its own (op_scratch.h: freed on every path) and calls the production launchers of sepformer.h unchanged.  The product path does not come here.
#include <algorithm>
#include <vector>
#include "../../include/ccx.h"
#include "ccx_common.h"
#include "op_scratch.h"
#include "sepformer.h"

// a device buffer: present, 16-byte aligned, at least `need` elements stated
#define SEP_BUF(field, need)                                                                                                        \
  do {                                                                                                                              \
    CCX_REQUIRE(ctx, d->field != nullptr, "ccx_sep_op: %s is NULL", #field);                                                        \
    CCX_REQUIRE(ctx, ccx_aligned16(d->field), "ccx_sep_op: %s is not 16-byte aligned", #field);                                         \
    CCX_REQUIRE(ctx, d->field##_elems >= (int64_t)(need), "ccx_sep_op: %s is accessed up to element %ld, %s_elems=%ld", #field,     \
                (long)(need), #field, (long)d->field##_elems);                                                                      \
  } while (0)
// a parameter tensor: present, aligned, exactly `count` elements (`efield`: the count's field)
#define SEP_PARAM(field, efield, count)                                                                                             \
  do {                                                                                                                              \
    CCX_REQUIRE(ctx, d->field != nullptr, "ccx_sep_op: %s is NULL", #field);                                                        \
    CCX_REQUIRE(ctx, ccx_aligned16(d->field), "ccx_sep_op: %s is not 16-byte aligned", #field);                                         \
    CCX_REQUIRE(ctx, d->efield == (int64_t)(count), "ccx_sep_op: %s holds %ld elements (%s), the kernel reads %ld", #field,         \
                (long)d->efield, #efield, (long)(count));                                                                           \
  } while (0)
#define SEP_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ccx_fail(ctx, CCX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

extern "C" int ccx_sep_op(ccx_ctx* ctx, int op, const ccx_sep_desc* d, void* stream_) {
  if (!ctx) return CCX_ERR_ARG;
  hipStream_t st = (hipStream_t)stream_;
  CCX_REQUIRE(ctx, d != nullptr, "ccx_sep_op: desc is NULL");
  CCX_REQUIRE(ctx, op >= CCX_SEP_ATTN_BLOCK && op <= CCX_SEP_DECODER, "ccx_sep_op: unknown op %d", op);
  const int rows = d->rows;
  CCX_REQUIRE(ctx, rows >= 1 && rows <= (1 << 24), "ccx_sep_op: rows = %d out of range [1, 2^24]", rows);
  const bool seq_op = op == CCX_SEP_ATTN_BLOCK || op == CCX_SEP_ATTENTION || op == CCX_SEP_FINAL_NORM;
  int max_len = 0;
  if (seq_op) {
    CCX_REQUIRE(ctx, d->n_seq >= 1 && d->n_seq <= (1 << 20), "ccx_sep_op: n_seq = %d out of range [1, 2^20]", d->n_seq);
    CCX_REQUIRE(ctx, d->seq_start && d->seq_len, "ccx_sep_op: seq_start or seq_len is NULL");
    for (int i = 0; i < d->n_seq; i++) {
      const int s0 = d->seq_start[i], len = d->seq_len[i];
      CCX_REQUIRE(ctx, len >= 1, "ccx_sep_op: seq_len[%d] = %d, a sequence needs at least one token", i, len);
      CCX_REQUIRE(ctx, s0 >= 0 && s0 <= rows && len <= rows - s0, "ccx_sep_op: seq_start[%d] = %d, seq_len[%d] = %d leave the %d rows", i, s0, i,
                  len, rows);
      if (op == CCX_SEP_ATTN_BLOCK)
        CCX_REQUIRE(ctx, len <= CCX_SEP_FUSED_MAX_TOK, "ccx_sep_op: seq_len[%d] = %d, the fused attention block holds at most %d tokens", i, len,
                    CCX_SEP_FUSED_MAX_TOK);
      max_len = std::max(max_len, len);
    }
    if (op == CCX_SEP_ATTN_BLOCK) {     // in place: two blocks must not own the same row
      std::vector<std::pair<int, int>> iv(d->n_seq);
      for (int i = 0; i < d->n_seq; i++) iv[i] = {d->seq_start[i], i};
      std::sort(iv.begin(), iv.end());
      for (int i = 1; i < d->n_seq; i++) {
        const int a = iv[i - 1].second, b = iv[i].second;
        CCX_REQUIRE(ctx, d->seq_start[a] + d->seq_len[a] <= d->seq_start[b], "ccx_sep_op: seq_start / seq_len: sequences %d and %d overlap (written in place)", a, b);
      }
    }
  }
  const int64_t tok128 = (int64_t)rows * 128;
  CCX_REQUIRE(ctx, op != CCX_SEP_DECODER || (d->n_spk >= 0 && d->n_spk <= 4), "ccx_sep_op: n_spk = %d out of range [1, 4] (0 means 2)", d->n_spk);
  const int n_spk = d->n_spk == 0 ? 2 : d->n_spk;      // op 4 only
  switch (op) {
    case CCX_SEP_ATTN_BLOCK:
      SEP_BUF(h, tok128);
      SEP_PARAM(ln_g, ln_elems, 128); SEP_PARAM(ln_b, ln_elems, 128);
      SEP_PARAM(wqkv, wqkv_elems, 384 * 128); SEP_PARAM(bqkv, bqkv_elems, 384);
      SEP_PARAM(wo, wo_elems, 128 * 128); SEP_PARAM(bo, bo_elems, 128);
      break;
    case CCX_SEP_ATTENTION:
      SEP_BUF(qkv, (int64_t)rows * 384);
      SEP_BUF(att, tok128);
      break;
    case CCX_SEP_FFN:
      CCX_REQUIRE(ctx, d->d_ffn >= 64 && d->d_ffn <= 1024 && d->d_ffn % 64 == 0, "ccx_sep_op: d_ffn = %d must be a multiple of 64 in [64, 1024]", d->d_ffn);
      CCX_REQUIRE(ctx, d->n_tok >= 1 && d->n_tok <= rows, "ccx_sep_op: n_tok = %d out of range [1, rows = %d]", d->n_tok, rows);
      SEP_BUF(h, tok128);
      SEP_PARAM(ln_g, ln_elems, 128); SEP_PARAM(ln_b, ln_elems, 128);
      SEP_PARAM(w1, w1_elems, (int64_t)d->d_ffn * 128); SEP_PARAM(b1, b1_elems, d->d_ffn);
      SEP_PARAM(w2, w2_elems, (int64_t)d->d_ffn * 128); SEP_PARAM(b2, b2_elems, 128);
      break;
    case CCX_SEP_FINAL_NORM:
      SEP_BUF(h, tok128); SEP_BUF(xin, tok128); SEP_BUF(y, tok128);
      CCX_REQUIRE(ctx, d->y != d->h && d->y != d->xin, "ccx_sep_op: y aliases h or xin");
      SEP_PARAM(ln_g, ln_elems, 128); SEP_PARAM(ln_b, ln_elems, 128);
      SEP_PARAM(gln_g, gln_elems, 128); SEP_PARAM(gln_b, gln_elems, 128);
      break;
    default: {  // CCX_SEP_DECODER
      CCX_REQUIRE(ctx, d->n_utt >= 1 && d->n_utt <= 65535, "ccx_sep_op: n_utt = %d out of range [1, 65535]", d->n_utt);
      CCX_REQUIRE(ctx, d->segment >= 1, "ccx_sep_op: segment = %d must be positive", d->segment);
      CCX_REQUIRE(ctx, d->out_stride >= 16 && d->out_stride <= (1 << 30), "ccx_sep_op: out_stride = %ld out of range [16, 2^30]", (long)d->out_stride);
      CCX_REQUIRE(ctx, d->utt_tok0 && d->utt_L && d->utt_T, "ccx_sep_op: utt_tok0, utt_L or utt_T is NULL");
      for (int u = 0; u < d->n_utt; u++) {
        const int L = d->utt_L[u], T = d->utt_T[u], t0 = d->utt_tok0[u];
        CCX_REQUIRE(ctx, L >= 1, "ccx_sep_op: utt_L[%d] = %d, an utterance needs at least one frame", u, L);
        CCX_REQUIRE(ctx, T >= 16 && T <= d->out_stride, "ccx_sep_op: utt_T[%d] = %d out of range [16, out_stride = %ld]", u, T, (long)d->out_stride);
        // the model's layout rule, not a read of the kernel: sep_decoder_kernel touches rows tok0 .. tok0 + L - 1 only, the chunk
        // padding behind them is the utterance's to own so that two utterances never share a chunk
        const int64_t padded = (int64_t)L + (d->segment - L % d->segment);
        CCX_REQUIRE(ctx, t0 >= 0 && t0 + padded <= rows, "ccx_sep_op: utt_tok0[%d] = %d with %ld chunk-padded frames leaves the %d rows", u, t0, (long)padded,
                    rows);
      }
      SEP_BUF(feats, tok128);
      SEP_BUF(fc, (int64_t)rows * 128 * n_spk);
      SEP_PARAM(wdec, wdec_elems, 128 * 16);
      SEP_BUF(out, (int64_t)d->n_utt * d->out_stride * n_spk);
    }
  }

  ccx_op_scratch sc;
  int *d_a = nullptr, *d_b = nullptr, *d_c = nullptr;
  if (seq_op) {
    SEP_HIP(sc.upload(&d_a, d->seq_start, (size_t)d->n_seq));
    SEP_HIP(sc.upload(&d_b, d->seq_len, (size_t)d->n_seq));
  } else if (op == CCX_SEP_DECODER) {
    SEP_HIP(sc.upload(&d_a, d->utt_tok0, (size_t)d->n_utt));
    SEP_HIP(sc.upload(&d_b, d->utt_L, (size_t)d->n_utt));
    SEP_HIP(sc.upload(&d_c, d->utt_T, (size_t)d->n_utt));
  }
  int rc = CCX_OK;
  switch (op) {
    case CCX_SEP_ATTN_BLOCK:
      rc = ccx_launch_sep_attn_block(ctx, (float*)d->h, (const float*)d->ln_g, (const float*)d->ln_b, (const bf16_t*)d->wqkv, (const float*)d->bqkv,
                                     (const bf16_t*)d->wo, (const float*)d->bo, d_a, d_b, d->n_seq, rows, max_len, st);
      break;
    case CCX_SEP_ATTENTION:
      rc = ccx_launch_sep_attention(ctx, (const bf16_t*)d->qkv, d_a, d_b, d->n_seq, 8, (bf16_t*)d->att, st);
      break;
    case CCX_SEP_FFN:
      rc = ccx_launch_sep_ffn(ctx, (float*)d->h, (const float*)d->ln_g, (const float*)d->ln_b, (const bf16_t*)d->w1, (const float*)d->b1,
                              (const bf16_t*)d->w2, (const float*)d->b2, d->n_tok, d->d_ffn, st);
      break;
    case CCX_SEP_FINAL_NORM:
      rc = ccx_launch_sep_final_norm(ctx, (const float*)d->h, (const float*)d->xin, d_a, d_b, d->n_seq, (const float*)d->ln_g, (const float*)d->ln_b,
                                     (const float*)d->gln_g, (const float*)d->gln_b, (float*)d->y, st);
      break;
    default:
      rc = ccx_launch_sep_decoder(ctx, (const float*)d->feats, (const float*)d->fc, d_a, d_b, d_c, (const float*)d->wdec, (float*)d->out,
                                  (long)d->out_stride, d->n_utt, n_spk, st);
  }
  SEP_HIP(hipStreamSynchronize(st));      // the scratch is freed on return
  return rc;
}
